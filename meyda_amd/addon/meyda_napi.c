/*
 * meyda_napi.c — N-API bridge between JavaScript typed arrays and the C ABI
 * (include/meyda_gpu.h). Thin by design: argument marshalling, typed-array
 * allocation and error translation; all compute is in libmeyda_gpu.so.
 *
 * Exports:
 *   createPlan(opts)                     -> plan handle (external; destroyed by GC or destroyPlan);
 *                                           opts.devices = [d0, d1, ...] makes a multi-device
 *                                           plan: batches are sharded over the devices and the
 *                                           features gathered to d0 by RCCL (mgx_group_*)
 *   destroyPlan(plan)
 *   planBusy(plan)                       -> true while an async extraction owns the plan
 *   extract(plan, frames, features)      -> { name: TypedArray }   (synchronous)
 *   extractAsync(plan, frames, features) -> Promise<{ name: TypedArray }>  (napi_async_work)
 *   extractWav(plan, wavBytes, features[, channel]) / extractWavAsync(...)
 *                                        -> the features of every full buffer of a .wav file;
 *                                           the raw PCM is decoded on the device
 *   summarizeGather(plan, samples, starts, frameOffsets, features[, {deltaWidth, deltaOrder, flux}]) / summarizeGatherAsync(...)
 *     flux: [{field, mode, lag, perFrame}] (numbers as in mgx_flux_request); the result gains `flux`, one
 *     {summary: Float64Array(nsignals x 4), perFrame: Float32Array(nframes)} per request
 *                                        -> { name: Float64Array(S x 4 x width) }: mean, variance, min, max
 *                                           of each field over every signal's buffers (mgx_summarize_host)
 *   onsetsGather(plan, samples, starts, frameOffsets, {field, mode, lag, preMax, postMax, preAvg, postAvg, delta, wait,
 *     envelope}) / onsetsGatherAsync(...)
 *                                        -> { onsetOffsets: Float64Array(S + 1), onsets: Float64Array(total)[, envelope:
 *                                           Float32Array(nframes)] }: the peaks of the field's flux within every
 *                                           signal, picked on the device (mgx_onsets_host)
 *   chromaWeights(bufferSize, sampleRate[, {numChroma, a440, centerOctave, octaveWidth, baseC}])
 *                                        -> Float32Array(numChroma x bufferSize / 2): the chroma filter bank
 *                                           (mgx_chroma_weights; host only)
 *   chromaGather(plan, samples, starts, frameOffsets | null, {weights, numChroma, norm, summary}) / chromaGatherAsync(...)
 *                                        -> { chroma: Float32Array(nframes x numChroma), numChroma[, summary:
 *                                           Float64Array(S x 4 x numChroma)] }: the chroma rows of every buffer,
 *                                           computed on the device from spectra that stay there (mgx_chroma_host)
 *   hpssGather(plan, samples, starts, frameOffsets | null, {kernelTime, kernelFreq, mode, marginHarmonic,
 *              marginPercussive, harmonic, percussive, chroma: {weights, numChroma, norm, perFrame, summary},
 *              flux: {mode, lag, perFrame, summary}}) / hpssGatherAsync(...)
 *                                        -> { [harmonic, percussive: Float32Array(nframes x bufferSize / 2)]
 *                                           [, chroma, numChroma, chromaSummary][, flux, fluxSummary] }: the median-filter
 *                                           harmonic / percussive split of every buffer's amplitude spectrum within its
 *                                           signal, the chroma of the harmonic rows and the flux of the percussive rows,
 *                                           computed on the device from spectra that stay there (mgx_hpss_host)
 *   tempogramWindow(winLength)           -> Float32Array(winLength): the periodic Hann window (mgx_tempogram_window; host only)
 *   tempoPrior(frameRate, numLags[, {startBpm, stdOctaves, maxBpm}])
 *                                        -> Float64Array(numLags): the log-normal tempo prior (mgx_tempo_prior; host only)
 *   beatTables(maxPeriod[, tightness])   -> {gauss: Float32Array, penalty: Float64Array}: the tables of the beat tracker
 *                                           (mgx_beat_tables; host only)
 *   beatsGather(plan, samples, starts, frameOffsets, {tempoGather's options but mean, gauss, penalty, maxPeriod, trim})
 *     / beatsGatherAsync(...)            -> {lag, numLags, beatOffsets, beats[, envelope]}: tempoGather's route and the
 *                                           beats of every signal at its lag, tracked on the device (mgx_beats_host)
 *   tempoGather(plan, samples, starts, frameOffsets, {field, mode, lag, winLength, numLags, norm, gain, window, prior,
 *               mean, envelope}) / tempoGatherAsync(...)
 *                                        -> { lag: Uint32Array(S), numLags[, summary: Float64Array(S x 4 x numLags)][,
 *                                           envelope: Float32Array(nframes)] }: the lag the prior picks from every
 *                                           signal's mean tempogram row, on the device (mgx_tempo_host)
 *   wavParse(wavBytes)                   -> { pcmFormat, channels, sampleRate, bitsPerSample, ... }
 *   hostTables(opts)                     -> { hanning, hamming, window, barkScale, barkLimits, melBins, dct }
 *   isPowerOfTwo(n), deviceCount(), featureNames(), featureInfo(name), abiVersion()
 * Feature names are the reference extractor names (src/extractors/index.js).
 * Scalars come back as Float64Array (JS numbers are doubles), vectors as Float32Array.
 */
#define NAPI_VERSION 4
#include <node_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/meyda_gpu.h"

#define CHECK(call)                                                       \
  do {                                                                    \
    if ((call) != napi_ok) {                                              \
      napi_throw_error(env, NULL, "meyda_napi: N-API call failed: " #call); \
      return NULL;                                                        \
    }                                                                     \
  } while (0)

static napi_value throw_mgx(napi_env env, int rc) {
  char code[16];
  snprintf(code, sizeof code, "%d", rc);
  napi_throw_error(env, code, mgx_last_error());
  return NULL;
}

typedef struct {
  mgx_plan* plan;
  mgx_group* group;  /* createPlan({devices: [...]}): a multi-device group */
  mgx_plan_desc desc;
  int busy;       /* an async extraction owns the plan */
  int finalized;  /* the JS handle was collected while busy: async_complete frees the box */
} plan_box;

static void plan_box_free(plan_box* b) {
  if (b->plan) mgx_plan_destroy(b->plan);
  if (b->group) mgx_group_destroy(b->group);
  free(b);
}

/* A queued or running async job holds a reference to the plan's external, so the GC
 * cannot collect it mid-job; `finalized` covers a finalizer that runs anyway while the
 * job is in flight (environment teardown): the box is then freed by async_complete. */
static void plan_finalize(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  plan_box* b = (plan_box*)data;
  if (b->busy) {
    b->finalized = 1;
    return;
  }
  plan_box_free(b);
}

static int get_u32_prop(napi_env env, napi_value obj, const char* name, uint32_t* out) {
  bool has = false;
  if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
  napi_value v;
  napi_valuetype t;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
  napi_typeof(env, v, &t);
  if (t != napi_number) return 0;
  napi_get_value_uint32(env, v, out);
  return 1;
}

static int get_f64_prop(napi_env env, napi_value obj, const char* name, double* out) {
  bool has = false;
  if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
  napi_value v;
  napi_valuetype t;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
  napi_typeof(env, v, &t);
  if (t != napi_number) return 0;
  napi_get_value_double(env, v, out);
  return 1;
}

static int get_str_prop(napi_env env, napi_value obj, const char* name, char* buf, size_t cap) {
  bool has = false;
  if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return 0;
  napi_value v;
  napi_valuetype t;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
  napi_typeof(env, v, &t);
  if (t != napi_string) return 0;
  size_t len = 0;
  napi_get_value_string_utf8(env, v, buf, cap, &len);
  return 1;
}

/* opts: { bufferSize, sampleRate, windowingFunction, precision, mode, numMelBands,
 *         numMfccCoeffs, device, scalarF64, dctSequential, mfccReferenceOrder, resident, devices } */
static int desc_from_opts(napi_env env, napi_value opts, mgx_plan_desc* d) {
  mgx_plan_desc_init(d);
  d->scalar_f64 = 1;
  double dv;
  uint32_t u;
  char s[64];
  if (get_f64_prop(env, opts, "bufferSize", &dv)) {
    if (!mgx_is_power_of_two(dv)) d->buffer_size = 3; /* reported as not-a-power-of-two */
    else d->buffer_size = (uint32_t)dv;
  }
  if (get_f64_prop(env, opts, "sampleRate", &dv)) d->sample_rate = dv;
  if (get_str_prop(env, opts, "windowingFunction", s, sizeof s)) {
    if (strcmp(s, "hanning") == 0) d->window = MGX_WINDOW_HANNING;
    else if (strcmp(s, "hamming") == 0) d->window = MGX_WINDOW_HAMMING;
    else d->window = 99;
  }
  if (get_str_prop(env, opts, "precision", s, sizeof s)) d->precision = strcmp(s, "fast") == 0 ? MGX_PRECISION_FAST : MGX_PRECISION_FAITHFUL;
  if (get_str_prop(env, opts, "mode", s, sizeof s)) d->mode = strcmp(s, "literal") == 0 ? MGX_MODE_LITERAL : MGX_MODE_PER_BUFFER_FFT;
  if (get_u32_prop(env, opts, "numMelBands", &u)) d->num_mel_bands = u;
  if (get_u32_prop(env, opts, "numMfccCoeffs", &u)) d->num_mfcc_coeffs = u;
  if (get_u32_prop(env, opts, "device", &u)) d->device = (int32_t)u;
  if (get_u32_prop(env, opts, "scalarF64", &u)) d->scalar_f64 = u ? 1 : 0;
  if (get_u32_prop(env, opts, "dctSequential", &u) && u) d->flags |= MGX_FLAG_DCT_SEQUENTIAL;
  if (get_u32_prop(env, opts, "mfccReferenceOrder", &u) && u) d->flags |= MGX_FLAG_MFCC_REFERENCE;
  if (get_u32_prop(env, opts, "resident", &u) && u) d->flags |= MGX_FLAG_RESIDENT;
  return 1;
}

static napi_value create_plan(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 1) {
    napi_throw_type_error(env, NULL, "createPlan(opts) expects an options object");
    return NULL;
  }
  mgx_plan_desc d;
  desc_from_opts(env, argv[0], &d);
  /* devices: [d0, d1, ...] shards every batch over those devices (d0 is the root) */
  int32_t devs[64];
  uint32_t ndev = 0;
  bool has = false, is_arr = false;
  napi_has_named_property(env, argv[0], "devices", &has);
  if (has) {
    napi_value arr;
    CHECK(napi_get_named_property(env, argv[0], "devices", &arr));
    napi_is_array(env, arr, &is_arr);
    if (is_arr) {
      napi_get_array_length(env, arr, &ndev);
      if (ndev == 0 || ndev > 64) {
        napi_throw_range_error(env, NULL, "devices must list 1 to 64 device ordinals");
        return NULL;
      }
      for (uint32_t i = 0; i < ndev; ++i) {
        napi_value v;
        int32_t dv = -1;
        napi_get_element(env, arr, i, &v);
        if (napi_get_value_int32(env, v, &dv) != napi_ok) {
          napi_throw_type_error(env, NULL, "devices must be numbers");
          return NULL;
        }
        devs[i] = dv;
      }
      d.device = devs[0];
    }
  }
  mgx_plan* p = NULL;
  mgx_group* grp = NULL;
  int rc = ndev > 0 ? mgx_group_create(&d, devs, ndev, &grp) : mgx_plan_create(&d, &p);
  if (rc) return throw_mgx(env, rc);
  plan_box* b = (plan_box*)calloc(1, sizeof *b);
  b->plan = p;
  b->group = grp;
  b->desc = d;
  napi_value ext;
  CHECK(napi_create_external(env, b, plan_finalize, NULL, &ext));
  return ext;
}

static plan_box* get_plan(napi_env env, napi_value v) {
  void* data = NULL;
  if (napi_get_value_external(env, v, &data) != napi_ok || !data) {
    napi_throw_type_error(env, NULL, "expected a plan created by createPlan()");
    return NULL;
  }
  plan_box* b = (plan_box*)data;
  if (!b->plan && !b->group) {
    napi_throw_error(env, NULL, "plan was destroyed");
    return NULL;
  }
  return b;
}

static napi_value plan_busy(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], r;
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  plan_box* b = argc ? get_plan(env, argv[0]) : NULL;
  if (!b) return NULL;
  CHECK(napi_get_boolean(env, b->busy != 0, &r));
  return r;
}

static napi_value destroy_plan(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  plan_box* b = argc ? get_plan(env, argv[0]) : NULL;
  if (!b) return NULL;
  if (b->busy) {
    napi_throw_error(env, NULL, "plan is busy with an async extraction");
    return NULL;
  }
  if (b->plan) mgx_plan_destroy(b->plan);
  if (b->group) mgx_group_destroy(b->group);
  b->plan = NULL;
  b->group = NULL;
  return NULL;
}

/* ------------------------------------------------------------ extraction job */
enum { SLOT_SCALAR0 = 0, SLOT_LOUD = MGX_NUM_SCALARS, SLOT_MFCC, SLOT_AMP, SLOT_POW, SLOT_CRE, SLOT_CIM, SLOT_MEL, NSLOTS };

/* The output fields, slot = field number: this file's copy of the library's table (meyda_amd/csrc/out_fields.h
 * out_field_bytes / out_field), kept because the addon is C against the public header alone. An output added
 * there is added here. Bytes per frame of field i: */
static size_t field_bytes(const mgx_plan_desc* d, int i) {
  const size_t n = d->buffer_size;
  const size_t floats[NSLOTS - SLOT_LOUD] = {d->num_bark_bands, d->num_mfcc_coeffs, n / 2, n / 2, n, n, d->num_mel_bands};
  return i < MGX_NUM_SCALARS ? (d->scalar_f64 ? 8u : 4u) : 4 * floats[i - SLOT_LOUD];
}
/* ... and its pointer in the caller's two structs */
static void set_field(mgx_outputs* o, mgx_aux_outputs* aux, int i, void* p) {
  float** const arrays[NSLOTS - SLOT_LOUD] = {&o->loudness_specific, &o->mfcc,         &o->amplitude_spectrum, &o->power_spectrum,
                                              &o->complex_real,      &o->complex_imag, &aux->mel_bands};
  if (i < MGX_NUM_SCALARS) o->scalars[i] = p;
  else *arrays[i - SLOT_LOUD] = (float*)p;
}

typedef struct {
  plan_box* box;
  const float* frames;
  uint64_t nframes;
  /* PCM input (extractWav): interleaved samples, decoded on the device */
  const unsigned char* pcm;
  uint64_t pcm_bytes;
  uint64_t pcm_frames;
  uint32_t pcm_format, pcm_channels, pcm_channel;
  /* hop > 0 (extractSignal, extractWav with a hop): `frames` is one contiguous signal of nsamples samples (or
   * the PCM's channel), cut into nframes = mgx_signal_frames() buffers that start every hop samples */
  uint32_t hop;
  uint64_t nsamples;
  /* extractGather: `frames` is nsamples samples, buffer f starts at starts[f] (malloc'd, nframes entries) */
  uint64_t* starts;
  int gather;
  /* summarizeGather: a gather job whose outputs are the signals' summaries (mgx_summary_outputs: per wanted
   * field nsignals x MGX_NUM_STATS x width doubles); signal s owns buffers [frame_offsets[s], frame_offsets[s + 1])
   * (malloc'd, nsignals + 1 entries). The per-frame rows stay on the device. */
  int summary;
  uint64_t* frame_offsets;
  uint64_t nsignals;
  mgx_summary_outputs sum;
  /* ... with the options {deltaWidth, deltaOrder}: the summaries of the rows' deltas (order 1) and of the deltas'
   * deltas (order 2) of the same fields beside them (mgx_summarize_deltas_host); delta_order 0: none asked for */
  uint32_t delta_width, delta_order;
  mgx_summary_outputs dsum[2];
  mgx_delta_summaries deltas;
  napi_ref drefs[2][NSLOTS];
  /* ... and with the option flux: the flux of the named fields pooled per signal, and per frame where asked
   * (mgx_summarize_flux_host); with flux and neither delta option no deltas are asked for */
  uint32_t num_flux;
  mgx_flux_request flux[MGX_FLUX_MAX_REQUESTS];
  int flux_per_frame[MGX_FLUX_MAX_REQUESTS];
  napi_ref frefs[2][MGX_FLUX_MAX_REQUESTS];  /* [0] the summaries, [1] the per-frame columns */
  /* onsetsGather: a gather job whose outputs are the peaks of flux[0]'s column within every signal (mgx_onsets_host);
   * peak_offsets: nsignals + 1 entries, peaks: nframes entries, which always hold them (both malloc'd) */
  int onsets;
  mgx_peak_params peak;
  uint64_t* peak_offsets;
  uint64_t* peaks;
  /* chromaGather: a gather job whose output is the chroma rows of every buffer under the caller's bank, and with
   * the option summary their pooling per signal (mgx_chroma_host); nsignals 0 and no table: the rows alone */
  int chroma;
  mgx_chroma_request creq;
  napi_ref crefs[3];  /* the bank (kept alive), the rows, the summaries */
  /* hpssGather: a gather job whose outputs are the harmonic and percussive parts of the amplitude rows, the chroma of
   * the harmonic part (creq, crefs) and the flux of the percussive part (flux[0], frefs[.][0]), each where asked for
   * (mgx_hpss_host) */
  int hpss;
  mgx_hpss_params hpar;
  int hchroma, hflux;
  float* hparts[2];
  napi_ref hrefs[2];  /* the harmonic rows, the percussive rows */
  /* tempoGather: a gather job whose outputs are the lag a tempo prior picks from the mean tempogram row of flux[0]'s
   * column within every signal, and with the option mean the pooled tempogram rows (mgx_tempo_host) */
  int tempo;
  mgx_tempo_params tpar;
  const float* twindow;
  const double* tprior;
  double* tsummary;
  uint32_t* tlag;
  napi_ref trefs[4];  /* the window and the prior (kept alive), the lags, the summaries */
  /* beatsGather: a tempo job with the tracker behind it (mgx_beats_host); peak_offsets and peaks as for onsetsGather */
  int beats;
  mgx_beat_params bpar;
  const float* bgauss;
  const double* bpenalty;
  napi_ref brefs[2];  /* the two tables (kept alive) */
  mgx_outputs out;
  mgx_aux_outputs aux;  /* melBands (SLOT_MEL): the job then makes the mgx_extract_*_ex call */
  /* The outputs are written straight into JS ArrayBuffers (napi_create_arraybuffer), held by
   * references until the result object takes them. (External ArrayBuffers over malloc'd memory
   * with a free finalizer made Node 12 abort at exit: v8impl ArrayBufferReference::Finalize's
   * assertion during the environment's teardown.) */
  napi_ref refs[NSLOTS];
  void* bufs[NSLOTS];
  size_t bytes[NSLOTS];
  int want[NSLOTS];
  napi_ref frames_ref;
  napi_ref plan_ref;  /* keeps the plan's external alive while the job is queued or running */
  napi_deferred deferred;
  napi_async_work work;
  int rc;
  char err[512];
} job;

static void job_free_buffers(napi_env env, job* j) {
  free(j->starts);
  j->starts = NULL;
  free(j->frame_offsets);
  j->frame_offsets = NULL;
  free(j->peak_offsets);
  j->peak_offsets = NULL;
  free(j->peaks);
  j->peaks = NULL;
  for (int i = 0; i < 3; ++i)
    if (j->crefs[i]) {
      napi_delete_reference(env, j->crefs[i]);
      j->crefs[i] = NULL;
    }
  for (int i = 0; i < 2; ++i)
    if (j->hrefs[i]) {
      napi_delete_reference(env, j->hrefs[i]);
      j->hrefs[i] = NULL;
    }
  for (int i = 0; i < 4; ++i)
    if (j->trefs[i]) {
      napi_delete_reference(env, j->trefs[i]);
      j->trefs[i] = NULL;
    }
  for (int i = 0; i < 2; ++i)
    if (j->brefs[i]) {
      napi_delete_reference(env, j->brefs[i]);
      j->brefs[i] = NULL;
    }
  for (int i = 0; i < NSLOTS; ++i)
    if (j->refs[i]) {
      napi_delete_reference(env, j->refs[i]);
      j->refs[i] = NULL;
      j->bufs[i] = NULL;
    }
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < NSLOTS; ++i)
      if (j->drefs[k][i]) {
        napi_delete_reference(env, j->drefs[k][i]);
        j->drefs[k][i] = NULL;
      }
  for (int k = 0; k < 2; ++k)
    for (int i = 0; i < MGX_FLUX_MAX_REQUESTS; ++i)
      if (j->frefs[k][i]) {
        napi_delete_reference(env, j->frefs[k][i]);
        j->frefs[k][i] = NULL;
      }
}

/* Parse the features argument (string or array of strings) into wanted output slots. */
static int parse_features(napi_env env, napi_value feats, job* j) {
  bool is_arr = false;
  napi_is_array(env, feats, &is_arr);
  uint32_t n = 1;
  if (is_arr) napi_get_array_length(env, feats, &n);
  for (uint32_t i = 0; i < n; ++i) {
    napi_value v = feats;
    if (is_arr) napi_get_element(env, feats, i, &v);
    char name[64];
    size_t len = 0;
    napi_valuetype t;
    napi_typeof(env, v, &t);
    if (t != napi_string) {
      napi_throw_type_error(env, NULL, "feature names must be strings");
      return 0;
    }
    napi_get_value_string_utf8(env, v, name, sizeof name, &len);
    int f = mgx_feature_index(name);
    if (f < 0) {
      char msg[128];
      snprintf(msg, sizeof msg, "unknown feature '%s'", name);
      napi_throw_type_error(env, NULL, msg);
      return 0;
    }
    if (j->summary && (f == MGX_COMPLEX_SPECTRUM || f == MGX_BUFFER)) {
      char msg[128];
      snprintf(msg, sizeof msg, "'%s' has no summary", name);
      napi_throw_type_error(env, NULL, msg);
      return 0;
    }
    if (f < MGX_NUM_SCALARS) j->want[f] = 1;
    else if (f == MGX_LOUDNESS) { j->want[SLOT_LOUD] = 1; j->want[MGX_LOUDNESS_TOTAL] = 1; }
    else if (f == MGX_MFCC) j->want[SLOT_MFCC] = 1;
    else if (f == MGX_AMPLITUDE_SPECTRUM) j->want[SLOT_AMP] = 1;
    else if (f == MGX_POWER_SPECTRUM) j->want[SLOT_POW] = 1;
    else if (f == MGX_COMPLEX_SPECTRUM) { j->want[SLOT_CRE] = 1; j->want[SLOT_CIM] = 1; }
    else if (f == MGX_MEL_BANDS) {
      if (j->box->group) {
        napi_throw_error(env, NULL, "melBands is not supported on a plan created with `devices`: device groups take no auxiliary outputs");
        return 0;
      }
      j->want[SLOT_MEL] = 1;
    }
    /* MGX_BUFFER is the input itself: handled by the JS facade */
  }
  return 1;
}

static int job_alloc(napi_env env, job* j, napi_value feats);

static int job_prepare(napi_env env, job* j, napi_value frames_v, napi_value feats) {
  bool is_ta = false;
  napi_is_typedarray(env, frames_v, &is_ta);
  if (!is_ta) {
    napi_throw_type_error(env, NULL, "frames must be a Float32Array");
    return 0;
  }
  napi_typedarray_type tt;
  size_t len = 0;
  void* data = NULL;
  napi_value ab;
  size_t off = 0;
  napi_get_typedarray_info(env, frames_v, &tt, &len, &data, &ab, &off);
  if (tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "frames must be a Float32Array");
    return 0;
  }
  const uint32_t n = j->box->desc.buffer_size;
  if (len % n) {
    napi_throw_range_error(env, NULL, "frames.length must be a multiple of bufferSize");
    return 0;
  }
  j->frames = (const float*)data;
  j->nframes = len / n;
  return job_alloc(env, j, feats);
}

/* hopSize: a positive integer that fits the C ABI's uint32. Plans created with `devices` (a group) take
 * dense buffers only (include/meyda_gpu.h). */
static int hop_of(napi_env env, job* j, napi_value v, uint32_t* hop) {
  napi_valuetype t = napi_undefined;
  double d = 0;
  napi_typeof(env, v, &t);
  if (t == napi_number) napi_get_value_double(env, v, &d);
  if (t != napi_number || !(d >= 1) || d > 4294967295.0 || d != (double)(uint64_t)d) {
    napi_throw_range_error(env, NULL, "hop must be a positive integer");
    return 0;
  }
  if (j->box->group) {
    napi_throw_error(env, NULL, "a hop is not supported on a plan created with `devices`: device groups take dense buffers only");
    return 0;
  }
  *hop = (uint32_t)d;
  return 1;
}

/* extractSignal(plan, samples, hop, features): one contiguous Float32Array, read in place at stride hop. */
static int job_prepare_signal(napi_env env, job* j, napi_value samples_v, napi_value hop_v, napi_value feats) {
  bool is_ta = false;
  napi_typedarray_type tt = napi_int8_array;
  size_t len = 0, off = 0;
  void* data = NULL;
  napi_value ab;
  napi_is_typedarray(env, samples_v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, samples_v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "samples must be a Float32Array");
    return 0;
  }
  if (!hop_of(env, j, hop_v, &j->hop)) return 0;
  j->frames = (const float*)data;
  j->nsamples = len;
  int rc = mgx_signal_frames(len, j->box->desc.buffer_size, j->hop, &j->nframes);
  if (rc) {
    throw_mgx(env, rc);
    return 0;
  }
  return job_alloc(env, j, feats);
}

/* A Float64Array of non-negative safe integers (sample indices, lengths) as uint64; `what` names it in the
 * RangeError. Returns a malloc'd array (NULL with an exception pending), *count entries (one at least is
 * allocated, so an empty table is not mistaken for a failure). */
static uint64_t* u64_of_f64(napi_env env, napi_value v, const char* what, size_t* count) {
  bool is_ta = false;
  napi_typedarray_type tt = napi_int8_array;
  size_t len = 0, off = 0;
  void* data = NULL;
  napi_value ab;
  char msg[128];
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float64_array) {
    snprintf(msg, sizeof msg, "%s must be a Float64Array", what);
    napi_throw_type_error(env, NULL, msg);
    return NULL;
  }
  uint64_t* out = (uint64_t*)malloc((len ? len : 1) * sizeof *out);
  if (!out) {
    napi_throw_error(env, NULL, "out of host memory");
    return NULL;
  }
  const double* d = (const double*)data;
  for (size_t i = 0; i < len; ++i) {
    if (!(d[i] >= 0) || d[i] > 9007199254740991.0 || d[i] != (double)(uint64_t)d[i]) {
      snprintf(msg, sizeof msg, "%s[%zu] must be a non-negative safe integer", what, i);
      free(out);
      napi_throw_range_error(env, NULL, msg);
      return NULL;
    }
    out[i] = (uint64_t)d[i];
  }
  *count = len;
  return out;
}

/* extractGather(plan, samples, starts, features): buffer f is samples [starts[f], starts[f] + bufferSize) of one
 * Float32Array; starts: a Float64Array of sample indices. */
static int job_prepare_gather(napi_env env, job* j, napi_value samples_v, napi_value starts_v, napi_value feats) {
  bool is_ta = false;
  napi_typedarray_type tt = napi_int8_array;
  size_t len = 0, off = 0, count = 0;
  void* data = NULL;
  napi_value ab;
  napi_is_typedarray(env, samples_v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, samples_v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "samples must be a Float32Array");
    return 0;
  }
  if (j->box->group) {
    napi_throw_error(env, NULL, "starts are not supported on a plan created with `devices`: device groups take dense buffers only");
    return 0;
  }
  j->starts = u64_of_f64(env, starts_v, "starts", &count);
  if (!j->starts) return 0;
  j->gather = 1;
  j->frames = (const float*)data;
  j->nsamples = len;
  j->nframes = count;
  return job_alloc(env, j, feats);
}

/* summarizeGather(plan, samples, starts, frameOffsets, features): extractGather's inputs and the table of the
 * signals' buffers (a Float64Array of nsignals + 1 offsets, as signalsFrameStarts returns it). */
/* A property of the options object as an integer in [lo, hi]; absent or undefined: dflt. 0 with a RangeError pending. */
static int option_u32(napi_env env, napi_value obj, const char* name, uint32_t lo, uint32_t hi, uint32_t dflt, uint32_t* out) {
  napi_value v;
  napi_valuetype t = napi_undefined;
  double d = 0;
  *out = dflt;
  if (napi_get_named_property(env, obj, name, &v) != napi_ok) return 0;
  napi_typeof(env, v, &t);
  if (t == napi_undefined) return 1;
  if (t == napi_number) napi_get_value_double(env, v, &d);
  if (t != napi_number || !(d >= lo) || d > hi || d != (double)(uint32_t)d) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s must be an integer from %u to %u", name, lo, hi);
    napi_throw_range_error(env, NULL, msg);
    return 0;
  }
  *out = (uint32_t)d;
  return 1;
}

/* Is the named property of obj there (neither absent nor undefined)? */
static int option_given(napi_env env, napi_value obj, const char* name, napi_value* v) {
  napi_valuetype t = napi_undefined;
  if (napi_get_named_property(env, obj, name, v) != napi_ok) return 0;
  napi_typeof(env, *v, &t);
  return t != napi_undefined;
}

/* The option flux: an array of 1 .. MGX_FLUX_MAX_REQUESTS objects {field, mode = 0, lag = 1, perFrame = false}.
 * The arrays are made once the numbers of buffers and signals are known (job_alloc_flux). */
static int parse_flux(napi_env env, job* j, napi_value arr) {
  bool is_arr = false;
  uint32_t n = 0;
  napi_is_array(env, arr, &is_arr);
  if (is_arr) napi_get_array_length(env, arr, &n);
  if (!is_arr || n < 1 || n > MGX_FLUX_MAX_REQUESTS) {
    napi_throw_range_error(env, NULL, "flux must be an array of 1 to 4 requests");
    return 0;
  }
  for (uint32_t i = 0; i < n; ++i) {
    napi_value e, pf;
    napi_valuetype t = napi_undefined;
    if (napi_get_element(env, arr, i, &e) == napi_ok) napi_typeof(env, e, &t);
    if (t != napi_object) {
      napi_throw_type_error(env, NULL, "a flux request must be an object: {field, mode, lag, perFrame}");
      return 0;
    }
    mgx_flux_request* r = &j->flux[i];
    r->struct_size = sizeof *r;
    if (!option_u32(env, e, "field", 0, MGX_NUM_FEATURES - 1, MGX_NUM_FEATURES, &r->field)) return 0;
    if (r->field == MGX_NUM_FEATURES) {
      napi_throw_type_error(env, NULL, "a flux request names its field");
      return 0;
    }
    if (!option_u32(env, e, "mode", 0, MGX_NUM_FLUX_MODES - 1, MGX_FLUX_RECTIFIED, &r->mode)) return 0;
    if (!option_u32(env, e, "lag", 1, MGX_FLUX_MAX_LAG, 1, &r->lag)) return 0;
    bool b = false;
    if (option_given(env, e, "perFrame", &pf)) napi_coerce_to_bool(env, pf, &pf), napi_get_value_bool(env, pf, &b);
    j->flux_per_frame[i] = b ? 1 : 0;
  }
  j->num_flux = n;
  return 1;
}

static int job_alloc_flux(napi_env env, job* j) {
  for (uint32_t i = 0; i < j->num_flux; ++i) {
    napi_value abv;
    void* data = NULL;
    /* (without signals there is nothing to pool: the library takes the per-frame column alone) */
    if (j->nsignals > 0) {
      if (napi_create_arraybuffer(env, (size_t)j->nsignals * MGX_NUM_STATS * sizeof(double), &data, &abv) != napi_ok ||
          napi_create_reference(env, abv, 1, &j->frefs[0][i]) != napi_ok) {
        napi_throw_error(env, NULL, "out of host memory");
        return 0;
      }
      j->flux[i].summary = (double*)data;
    }
    if (j->flux_per_frame[i]) {
      if (napi_create_arraybuffer(env, (size_t)j->nframes * sizeof(float), &data, &abv) != napi_ok ||
          napi_create_reference(env, abv, 1, &j->frefs[1][i]) != napi_ok) {
        napi_throw_error(env, NULL, "out of host memory");
        return 0;
      }
      memset(data, 0, (size_t)j->nframes * sizeof(float));
      j->flux[i].per_frame = (float*)data;
    }
  }
  return 1;
}

static int job_prepare_summary(napi_env env, job* j, napi_value samples_v, napi_value starts_v, napi_value offsets_v,
                               napi_value feats, napi_value options_v) {
  size_t count = 0;
  j->summary = 1;
  j->sum.struct_size = sizeof j->sum;
  napi_valuetype ot = napi_undefined;
  if (options_v) napi_typeof(env, options_v, &ot);
  napi_value fv, dv;
  const int has_flux = ot == napi_object && option_given(env, options_v, "flux", &fv);
  if (has_flux && !parse_flux(env, j, fv)) return 0;
  if (has_flux && !option_given(env, options_v, "deltaWidth", &dv) && !option_given(env, options_v, "deltaOrder", &dv)) {
    /* flux and no delta key: no deltas */
  } else if (ot == napi_object) {  /* the trailing options: {deltaWidth = 2, deltaOrder = 2} */
    if (!option_u32(env, options_v, "deltaWidth", 1, MGX_DELTA_MAX_WIDTH, 2, &j->delta_width)) return 0;
    if (!option_u32(env, options_v, "deltaOrder", 1, 2, 2, &j->delta_order)) return 0;
    j->deltas.struct_size = sizeof j->deltas;
    j->deltas.width = j->delta_width;
    for (uint32_t k = 0; k < j->delta_order; ++k) j->dsum[k].struct_size = sizeof j->dsum[k];
    j->deltas.delta = &j->dsum[0];
    j->deltas.delta2 = j->delta_order > 1 ? &j->dsum[1] : NULL;
  } else if (ot != napi_undefined && ot != napi_null) {
    napi_throw_type_error(env, NULL, "options must be an object: {deltaWidth, deltaOrder}");
    return 0;
  }
  j->frame_offsets = u64_of_f64(env, offsets_v, "frameOffsets", &count);
  if (!j->frame_offsets) return 0;
  if (count < 1) {
    napi_throw_range_error(env, NULL, "frameOffsets holds one entry more than there are signals");
    return 0;
  }
  j->nsignals = count - 1;
  return job_prepare_gather(env, j, samples_v, starts_v, feats) && job_alloc_flux(env, j);
}

/* onsetsGather(plan, samples, starts, frameOffsets, options): summarizeGather's inputs; options: {field, mode = 0,
 * lag = 1, preMax = 0, postMax = 0, preAvg = 0, postAvg = 0, delta = 0, wait = 0, envelope = false}. */
static int job_prepare_onsets(napi_env env, job* j, napi_value samples_v, napi_value starts_v, napi_value offsets_v,
                              napi_value options_v) {
  napi_valuetype ot = napi_undefined;
  napi_typeof(env, options_v, &ot);
  if (ot != napi_object) {
    napi_throw_type_error(env, NULL, "options must be an object: {field, mode, lag, preMax, postMax, preAvg, postAvg, delta, wait, envelope}");
    return 0;
  }
  j->onsets = 1;
  mgx_flux_request* r = &j->flux[0];
  r->struct_size = sizeof *r;
  if (!option_u32(env, options_v, "field", 0, MGX_NUM_FEATURES - 1, MGX_NUM_FEATURES, &r->field)) return 0;
  if (r->field == MGX_NUM_FEATURES) {
    napi_throw_type_error(env, NULL, "the onsets' flux names its field");
    return 0;
  }
  if (!option_u32(env, options_v, "mode", 0, MGX_NUM_FLUX_MODES - 1, MGX_FLUX_RECTIFIED, &r->mode)) return 0;
  if (!option_u32(env, options_v, "lag", 1, MGX_FLUX_MAX_LAG, 1, &r->lag)) return 0;
  mgx_peak_params* pp = &j->peak;
  pp->struct_size = sizeof *pp;
  if (!option_u32(env, options_v, "preMax", 0, MGX_PEAK_MAX_REACH, 0, &pp->pre_max)) return 0;
  if (!option_u32(env, options_v, "postMax", 0, MGX_PEAK_MAX_REACH, 0, &pp->post_max)) return 0;
  if (!option_u32(env, options_v, "preAvg", 0, MGX_PEAK_MAX_REACH, 0, &pp->pre_avg)) return 0;
  if (!option_u32(env, options_v, "postAvg", 0, MGX_PEAK_MAX_REACH, 0, &pp->post_avg)) return 0;
  if (!option_u32(env, options_v, "wait", 0, 4294967295u, 0, &pp->wait)) return 0;
  napi_value v;
  if (option_given(env, options_v, "delta", &v)) {
    napi_valuetype t = napi_undefined;
    napi_typeof(env, v, &t);
    if (t != napi_number) {
      napi_throw_type_error(env, NULL, "delta must be a number");
      return 0;
    }
    napi_get_value_double(env, v, &pp->delta);
    if (pp->delta != pp->delta) {
      napi_throw_range_error(env, NULL, "delta must not be NaN");
      return 0;
    }
  }
  bool b = false;
  if (option_given(env, options_v, "envelope", &v)) napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &b);
  j->flux_per_frame[0] = b ? 1 : 0;
  size_t count = 0, len = 0, off = 0;
  j->frame_offsets = u64_of_f64(env, offsets_v, "frameOffsets", &count);
  if (!j->frame_offsets) return 0;
  if (count < 2) {
    napi_throw_range_error(env, NULL, "frameOffsets holds one entry more than there are signals, and onsets need a signal");
    return 0;
  }
  j->nsignals = count - 1;
  bool is_ta = false;
  napi_typedarray_type tt = napi_int8_array;
  void* data = NULL;
  napi_value ab;
  napi_is_typedarray(env, samples_v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, samples_v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "samples must be a Float32Array");
    return 0;
  }
  if (j->box->group) {
    napi_throw_error(env, NULL, "starts are not supported on a plan created with `devices`: device groups take dense buffers only");
    return 0;
  }
  j->starts = u64_of_f64(env, starts_v, "starts", &count);
  if (!j->starts) return 0;
  j->gather = 1;
  j->frames = (const float*)data;
  j->nsamples = len;
  j->nframes = count;
  j->peak_offsets = (uint64_t*)calloc(j->nsignals + 1, sizeof(uint64_t));
  j->peaks = (uint64_t*)calloc(j->nframes ? j->nframes : 1, sizeof(uint64_t));
  if (!j->peak_offsets || !j->peaks) {
    napi_throw_error(env, NULL, "out of host memory");
    return 0;
  }
  if (j->flux_per_frame[0]) {
    if (napi_create_arraybuffer(env, (size_t)j->nframes * sizeof(float), &data, &ab) != napi_ok ||
        napi_create_reference(env, ab, 1, &j->frefs[1][0]) != napi_ok) {
      napi_throw_error(env, NULL, "out of host memory");
      return 0;
    }
    memset(data, 0, (size_t)j->nframes * sizeof(float));
    r->per_frame = (float*)data;
  }
  return 1;
}

/* A property of the options object as a finite double; absent or undefined: *out as it stands. 0 with an error pending. */
static int option_f64(napi_env env, napi_value obj, const char* name, double* out) {
  napi_value v;
  if (!option_given(env, obj, name, &v)) return 1;
  napi_valuetype t = napi_undefined;
  double d = 0;
  napi_typeof(env, v, &t);
  if (t == napi_number) napi_get_value_double(env, v, &d);
  if (t != napi_number || d != d || d - d != 0) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s must be a finite number", name);
    napi_throw_range_error(env, NULL, msg);
    return 0;
  }
  *out = d;
  return 1;
}

/* chromaGather(plan, samples, starts, frameOffsets, options): extractGather's inputs, the table of the signals'
 * buffers or null (no signals: the rows alone), and options: {weights: a Float32Array of numChroma x bufferSize / 2,
 * numChroma, norm = 1 (0 none, 1 max), summary = false}. */
static int job_prepare_chroma(napi_env env, job* j, napi_value samples_v, napi_value starts_v, napi_value offsets_v,
                              napi_value options_v) {
  napi_valuetype ot = napi_undefined;
  napi_typeof(env, options_v, &ot);
  if (ot != napi_object) {
    napi_throw_type_error(env, NULL, "options must be an object: {weights, numChroma, norm, summary}");
    return 0;
  }
  j->chroma = 1;
  mgx_chroma_request* r = &j->creq;
  r->struct_size = sizeof *r;
  if (!option_u32(env, options_v, "numChroma", 1, MGX_CHROMA_MAX_BINS, 12, &r->num_chroma)) return 0;
  if (!option_u32(env, options_v, "norm", 0, MGX_NUM_CHROMA_NORMS - 1, MGX_CHROMA_NORM_MAX, &r->norm)) return 0;
  napi_value v, ab;
  bool want_summary = false, is_ta = false;
  if (option_given(env, options_v, "summary", &v)) napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &want_summary);
  napi_typedarray_type tt = napi_int8_array;
  size_t len = 0, off = 0, count = 0;
  void* data = NULL;
  if (option_given(env, options_v, "weights", &v)) napi_is_typedarray(env, v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "weights must be a Float32Array");
    return 0;
  }
  if (len != (size_t)r->num_chroma * (j->box->desc.buffer_size / 2)) {
    napi_throw_range_error(env, NULL, "weights.length must be numChroma x bufferSize / 2");
    return 0;
  }
  if (napi_create_reference(env, v, 1, &j->crefs[0]) != napi_ok) return 0;
  r->weights = (const float*)data;
  napi_typeof(env, offsets_v, &ot);
  if (ot != napi_undefined && ot != napi_null) {
    j->frame_offsets = u64_of_f64(env, offsets_v, "frameOffsets", &count);
    if (!j->frame_offsets) return 0;
    if (count < 1) {
      napi_throw_range_error(env, NULL, "frameOffsets holds one entry more than there are signals");
      return 0;
    }
    j->nsignals = count - 1;
  }
  if (want_summary && j->nsignals == 0) {
    napi_throw_range_error(env, NULL, "summary needs frameOffsets with a signal");
    return 0;
  }
  is_ta = false;
  napi_is_typedarray(env, samples_v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, samples_v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "samples must be a Float32Array");
    return 0;
  }
  if (j->box->group) {
    napi_throw_error(env, NULL, "starts are not supported on a plan created with `devices`: device groups take dense buffers only");
    return 0;
  }
  j->starts = u64_of_f64(env, starts_v, "starts", &count);
  if (!j->starts) return 0;
  j->gather = 1;
  j->frames = (const float*)data;
  j->nsamples = len;
  j->nframes = count;
  const size_t row_bytes = (size_t)j->nframes * r->num_chroma * sizeof(float);
  if (napi_create_arraybuffer(env, row_bytes, &data, &ab) != napi_ok || napi_create_reference(env, ab, 1, &j->crefs[1]) != napi_ok) {
    napi_throw_error(env, NULL, "out of host memory");
    return 0;
  }
  memset(data, 0, row_bytes);
  r->per_frame = (float*)data;
  if (want_summary) {
    if (napi_create_arraybuffer(env, (size_t)j->nsignals * MGX_NUM_STATS * r->num_chroma * sizeof(double), &data, &ab) != napi_ok ||
        napi_create_reference(env, ab, 1, &j->crefs[2]) != napi_ok) {
      napi_throw_error(env, NULL, "out of host memory");
      return 0;
    }
    r->summary = (double*)data;
  }
  return 1;
}

/* A new ArrayBuffer of `bytes` zero bytes, held by *ref. 0 with an error pending. */
static int zeroed_buffer(napi_env env, size_t bytes, napi_ref* ref, void** out) {
  napi_value ab;
  void* data = NULL;
  if (napi_create_arraybuffer(env, bytes, &data, &ab) != napi_ok || napi_create_reference(env, ab, 1, ref) != napi_ok) {
    napi_throw_error(env, NULL, "out of host memory");
    return 0;
  }
  memset(data, 0, bytes);
  *out = data;
  return 1;
}

/* A boolean property of the options object; absent or undefined: dflt. */
static bool option_bool(napi_env env, napi_value obj, const char* name, bool dflt) {
  napi_value v;
  bool b = dflt;
  if (option_given(env, obj, name, &v)) napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &b);
  return b;
}

/* hpssGather(plan, samples, starts, frameOffsets, options): extractGather's inputs, the table of the signals' buffers
 * or null (one signal: every buffer), and options: {kernelTime = 31, kernelFreq = 31 (odd, 1 .. 31), mode = 2 (0 medians,
 * 1 soft1, 2 soft2, 3 hard), marginHarmonic = 1, marginPercussive = 1 (>= 1), harmonic = false, percussive = false (the
 * rows themselves), chroma: {weights, numChroma, norm = 1, perFrame = true, summary = false} (of the harmonic rows),
 * flux: {mode = 0, lag = 1, perFrame = true, summary = false} (of the percussive rows)}; one output at least. */
static int job_prepare_hpss(napi_env env, job* j, napi_value samples_v, napi_value starts_v, napi_value offsets_v,
                            napi_value options_v) {
  napi_valuetype ot = napi_undefined;
  napi_typeof(env, options_v, &ot);
  if (ot != napi_object) {
    napi_throw_type_error(env, NULL, "options must be an object: {kernelTime, kernelFreq, mode, marginHarmonic, marginPercussive, harmonic, percussive, chroma, flux}");
    return 0;
  }
  j->hpss = 1;
  mgx_hpss_params* h = &j->hpar;
  mgx_hpss_params_init(h);
  const char* const kname[2] = {"kernelTime", "kernelFreq"};
  uint32_t* const kdst[2] = {&h->kernel_time, &h->kernel_freq};
  for (int i = 0; i < 2; ++i) {
    if (!option_u32(env, options_v, kname[i], 1, MGX_HPSS_MAX_KERNEL, MGX_HPSS_MAX_KERNEL, kdst[i])) return 0;
    if (!(*kdst[i] & 1u)) {
      char msg[64];
      snprintf(msg, sizeof msg, "%s must be odd", kname[i]);
      napi_throw_range_error(env, NULL, msg);
      return 0;
    }
  }
  if (!option_u32(env, options_v, "mode", 0, MGX_NUM_HPSS_MODES - 1, MGX_HPSS_SOFT2, &h->mode)) return 0;
  const char* const mname[2] = {"marginHarmonic", "marginPercussive"};
  float* const mdst[2] = {&h->margin_harmonic, &h->margin_percussive};
  for (int i = 0; i < 2; ++i) {
    double m = 1.0;
    if (!option_f64(env, options_v, mname[i], &m)) return 0;
    if (!(m >= 1.0) || (double)(float)m - (double)(float)m != 0) {
      char msg[64];
      snprintf(msg, sizeof msg, "%s must be a finite number >= 1", mname[i]);
      napi_throw_range_error(env, NULL, msg);
      return 0;
    }
    *mdst[i] = (float)m;
  }
  const bool want_part[2] = {option_bool(env, options_v, "harmonic", false), option_bool(env, options_v, "percussive", false)};
  napi_value cv, fv, v, ab;
  napi_typedarray_type tt = napi_int8_array;
  size_t len = 0, off = 0, count = 0;
  void* data = NULL;
  bool is_ta = false, chroma_rows = true, chroma_summary = false, flux_rows = true, flux_summary = false;
  const size_t cols = j->box->desc.buffer_size / 2;
  if (option_given(env, options_v, "chroma", &cv)) {
    napi_typeof(env, cv, &ot);
    if (ot != napi_object) {
      napi_throw_type_error(env, NULL, "chroma must be an object: {weights, numChroma, norm, perFrame, summary}");
      return 0;
    }
    j->hchroma = 1;
    mgx_chroma_request* r = &j->creq;
    r->struct_size = sizeof *r;
    if (!option_u32(env, cv, "numChroma", 1, MGX_CHROMA_MAX_BINS, 12, &r->num_chroma)) return 0;
    if (!option_u32(env, cv, "norm", 0, MGX_NUM_CHROMA_NORMS - 1, MGX_CHROMA_NORM_MAX, &r->norm)) return 0;
    chroma_rows = option_bool(env, cv, "perFrame", true);
    chroma_summary = option_bool(env, cv, "summary", false);
    if (option_given(env, cv, "weights", &v)) napi_is_typedarray(env, v, &is_ta);
    if (is_ta) napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off);
    if (!is_ta || tt != napi_float32_array) {
      napi_throw_type_error(env, NULL, "chroma.weights must be a Float32Array");
      return 0;
    }
    if (len != (size_t)r->num_chroma * cols) {
      napi_throw_range_error(env, NULL, "chroma.weights.length must be numChroma x bufferSize / 2");
      return 0;
    }
    if (!chroma_rows && !chroma_summary) {
      napi_throw_range_error(env, NULL, "chroma asks for neither perFrame nor summary");
      return 0;
    }
    if (napi_create_reference(env, v, 1, &j->crefs[0]) != napi_ok) return 0;
    r->weights = (const float*)data;
  }
  if (option_given(env, options_v, "flux", &fv)) {
    napi_typeof(env, fv, &ot);
    if (ot != napi_object) {
      napi_throw_type_error(env, NULL, "flux must be an object: {mode, lag, perFrame, summary}");
      return 0;
    }
    j->hflux = 1;
    mgx_flux_request* r = &j->flux[0];
    r->struct_size = sizeof *r;
    r->field = MGX_AMPLITUDE_SPECTRUM;
    if (!option_u32(env, fv, "mode", 0, MGX_NUM_FLUX_MODES - 1, MGX_FLUX_RECTIFIED, &r->mode)) return 0;
    if (!option_u32(env, fv, "lag", 1, MGX_FLUX_MAX_LAG, 1, &r->lag)) return 0;
    flux_rows = option_bool(env, fv, "perFrame", true);
    flux_summary = option_bool(env, fv, "summary", false);
    if (!flux_rows && !flux_summary) {
      napi_throw_range_error(env, NULL, "flux asks for neither perFrame nor summary");
      return 0;
    }
  }
  if (!want_part[0] && !want_part[1] && !j->hchroma && !j->hflux) {
    napi_throw_range_error(env, NULL, "nothing asked for: harmonic, percussive, chroma or flux");
    return 0;
  }
  napi_typeof(env, offsets_v, &ot);
  if (ot != napi_undefined && ot != napi_null) {
    j->frame_offsets = u64_of_f64(env, offsets_v, "frameOffsets", &count);
    if (!j->frame_offsets) return 0;
    if (count < 1) {
      napi_throw_range_error(env, NULL, "frameOffsets holds one entry more than there are signals");
      return 0;
    }
    j->nsignals = count - 1;
  }
  if (((j->hchroma && chroma_summary) || (j->hflux && flux_summary)) && j->nsignals == 0) {
    napi_throw_range_error(env, NULL, "summary needs frameOffsets with a signal");
    return 0;
  }
  is_ta = false;
  napi_is_typedarray(env, samples_v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, samples_v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "samples must be a Float32Array");
    return 0;
  }
  if (j->box->group) {
    napi_throw_error(env, NULL, "starts are not supported on a plan created with `devices`: device groups take dense buffers only");
    return 0;
  }
  j->starts = u64_of_f64(env, starts_v, "starts", &count);
  if (!j->starts) return 0;
  j->gather = 1;
  j->frames = (const float*)data;
  j->nsamples = len;
  j->nframes = count;
  for (int i = 0; i < 2; ++i)
    if (want_part[i] && !zeroed_buffer(env, (size_t)j->nframes * cols * sizeof(float), &j->hrefs[i], (void**)&j->hparts[i])) return 0;
  if (j->hchroma) {
    mgx_chroma_request* r = &j->creq;
    if (chroma_rows && !zeroed_buffer(env, (size_t)j->nframes * r->num_chroma * sizeof(float), &j->crefs[1], (void**)&r->per_frame)) return 0;
    if (chroma_summary &&
        !zeroed_buffer(env, (size_t)j->nsignals * MGX_NUM_STATS * r->num_chroma * sizeof(double), &j->crefs[2], (void**)&r->summary))
      return 0;
  }
  if (j->hflux) {
    mgx_flux_request* r = &j->flux[0];
    if (flux_rows && !zeroed_buffer(env, (size_t)j->nframes * sizeof(float), &j->frefs[1][0], (void**)&r->per_frame)) return 0;
    if (flux_summary && !zeroed_buffer(env, (size_t)j->nsignals * MGX_NUM_STATS * sizeof(double), &j->frefs[0][0], (void**)&r->summary))
      return 0;
  }
  return 1;
}

/* A typed-array property of the options object of the given type and length, kept alive by *ref. 0 with an error pending. */
static int option_typed(napi_env env, napi_value obj, const char* name, napi_typedarray_type want, size_t count, napi_ref* ref,
                        void** out) {
  napi_value v, ab;
  bool is_ta = false;
  napi_typedarray_type tt = napi_int8_array;
  size_t len = 0, off = 0;
  void* data = NULL;
  char msg[96];
  if (option_given(env, obj, name, &v)) napi_is_typedarray(env, v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != want) {
    snprintf(msg, sizeof msg, "%s must be a %s", name, want == napi_float32_array ? "Float32Array" : "Float64Array");
    napi_throw_type_error(env, NULL, msg);
    return 0;
  }
  if (len != count) {
    snprintf(msg, sizeof msg, "%s.length must be %zu", name, count);
    napi_throw_range_error(env, NULL, msg);
    return 0;
  }
  if (napi_create_reference(env, v, 1, ref) != napi_ok) return 0;
  *out = data;
  return 1;
}

/* tempoGather(plan, samples, starts, frameOffsets, options): summarizeGather's inputs; options: {field, mode = 0,
 * lag = 1, winLength = 384, numLags = winLength, norm = 1 (0 none, 1 lag0), gain = 1e6, window: a Float32Array of
 * winLength, prior: a Float64Array of numLags, mean = false, envelope = false}. */
/* beatsGather(plan, samples, starts, frameOffsets, options): the same, without mean, and {maxPeriod = max(numLags - 1, 1),
 * trim = true, gauss: a Float32Array of (maxPeriod + 1)(maxPeriod + 2) / 2, penalty: a Float64Array of (maxPeriod + 1)^2}. */
static int job_prepare_tempo(napi_env env, job* j, napi_value samples_v, napi_value starts_v, napi_value offsets_v,
                             napi_value options_v, int beats) {
  napi_valuetype ot = napi_undefined;
  napi_typeof(env, options_v, &ot);
  if (ot != napi_object) {
    napi_throw_type_error(env, NULL, beats ? "options must be an object: {field, mode, lag, winLength, numLags, norm, gain, window, prior, "
                                             "maxPeriod, trim, gauss, penalty, envelope}"
                                           : "options must be an object: {field, mode, lag, winLength, numLags, norm, gain, window, prior, mean, envelope}");
    return 0;
  }
  j->tempo = 1;
  j->beats = beats;
  mgx_flux_request* r = &j->flux[0];
  r->struct_size = sizeof *r;
  if (!option_u32(env, options_v, "field", 0, MGX_NUM_FEATURES - 1, MGX_NUM_FEATURES, &r->field)) return 0;
  if (r->field == MGX_NUM_FEATURES) {
    napi_throw_type_error(env, NULL, "the tempo's flux names its field");
    return 0;
  }
  if (!option_u32(env, options_v, "mode", 0, MGX_NUM_FLUX_MODES - 1, MGX_FLUX_RECTIFIED, &r->mode)) return 0;
  if (!option_u32(env, options_v, "lag", 1, MGX_FLUX_MAX_LAG, 1, &r->lag)) return 0;
  mgx_tempo_params* tp = &j->tpar;
  mgx_tempo_params_init(tp);
  if (!option_u32(env, options_v, "winLength", 2, MGX_TEMPOGRAM_MAX_WIN, tp->win_length, &tp->win_length)) return 0;
  if (!option_u32(env, options_v, "numLags", 1, tp->win_length, tp->win_length, &tp->num_lags)) return 0;
  if (!option_u32(env, options_v, "norm", 0, MGX_NUM_TEMPOGRAM_NORMS - 1, MGX_TEMPOGRAM_NORM_LAG0, &tp->norm)) return 0;
  if (!option_f64(env, options_v, "gain", &tp->gain)) return 0;
  if (tp->gain < 0) {
    napi_throw_range_error(env, NULL, "gain must not be negative");
    return 0;
  }
  void* data = NULL;
  if (!option_typed(env, options_v, "window", napi_float32_array, tp->win_length, &j->trefs[0], &data)) return 0;
  j->twindow = (const float*)data;
  if (!option_typed(env, options_v, "prior", napi_float64_array, tp->num_lags, &j->trefs[1], &data)) return 0;
  j->tprior = (const double*)data;
  napi_value v, ab;
  bool want_mean = false, b = false;
  if (beats) {
    mgx_beat_params* bp = &j->bpar;
    mgx_beat_params_init(bp);
    const uint32_t reach = tp->num_lags > 1 ? tp->num_lags - 1 : 1;  /* the largest lag there can be */
    if (!option_u32(env, options_v, "maxPeriod", reach, MGX_BEAT_MAX_PERIOD, reach, &bp->max_period)) return 0;
    bool trim = true;
    if (option_given(env, options_v, "trim", &v)) napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &trim);
    bp->trim = trim ? 1 : 0;
    const size_t P = bp->max_period;
    if (!option_typed(env, options_v, "gauss", napi_float32_array, (P + 1) * (P + 2) / 2, &j->brefs[0], &data)) return 0;
    j->bgauss = (const float*)data;
    if (!option_typed(env, options_v, "penalty", napi_float64_array, (P + 1) * (P + 1), &j->brefs[1], &data)) return 0;
    j->bpenalty = (const double*)data;
  } else if (option_given(env, options_v, "mean", &v)) {
    napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &want_mean);
  }
  if (option_given(env, options_v, "envelope", &v)) napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &b);
  j->flux_per_frame[0] = b ? 1 : 0;
  size_t count = 0, len = 0, off = 0;
  j->frame_offsets = u64_of_f64(env, offsets_v, "frameOffsets", &count);
  if (!j->frame_offsets) return 0;
  if (count < 2) {
    napi_throw_range_error(env, NULL, "frameOffsets holds one entry more than there are signals, and a tempo needs a signal");
    return 0;
  }
  j->nsignals = count - 1;
  bool is_ta = false;
  napi_typedarray_type tt = napi_int8_array;
  napi_is_typedarray(env, samples_v, &is_ta);
  if (is_ta) napi_get_typedarray_info(env, samples_v, &tt, &len, &data, &ab, &off);
  if (!is_ta || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "samples must be a Float32Array");
    return 0;
  }
  if (j->box->group) {
    napi_throw_error(env, NULL, "starts are not supported on a plan created with `devices`: device groups take dense buffers only");
    return 0;
  }
  j->starts = u64_of_f64(env, starts_v, "starts", &count);
  if (!j->starts) return 0;
  j->gather = 1;
  j->frames = (const float*)data;
  j->nsamples = len;
  j->nframes = count;
  if (napi_create_arraybuffer(env, (size_t)j->nsignals * sizeof(uint32_t), &data, &ab) != napi_ok ||
      napi_create_reference(env, ab, 1, &j->trefs[2]) != napi_ok) {
    napi_throw_error(env, NULL, "out of host memory");
    return 0;
  }
  memset(data, 0, (size_t)j->nsignals * sizeof(uint32_t));
  j->tlag = (uint32_t*)data;
  if (beats) {
    j->peak_offsets = (uint64_t*)calloc(j->nsignals + 1, sizeof(uint64_t));
    j->peaks = (uint64_t*)calloc(j->nframes ? j->nframes : 1, sizeof(uint64_t));
    if (!j->peak_offsets || !j->peaks) {
      napi_throw_error(env, NULL, "out of host memory");
      return 0;
    }
  }
  if (want_mean) {
    if (napi_create_arraybuffer(env, (size_t)j->nsignals * MGX_NUM_STATS * tp->num_lags * sizeof(double), &data, &ab) != napi_ok ||
        napi_create_reference(env, ab, 1, &j->trefs[3]) != napi_ok) {
      napi_throw_error(env, NULL, "out of host memory");
      return 0;
    }
    j->tsummary = (double*)data;
  }
  if (j->flux_per_frame[0]) {
    if (napi_create_arraybuffer(env, (size_t)j->nframes * sizeof(float), &data, &ab) != napi_ok ||
        napi_create_reference(env, ab, 1, &j->frefs[1][0]) != napi_ok) {
      napi_throw_error(env, NULL, "out of host memory");
      return 0;
    }
    memset(data, 0, (size_t)j->nframes * sizeof(float));
    r->per_frame = (float*)data;
  }
  return 1;
}

/* Field i of a summary (the complex spectrum has none) */
static void set_summary_field(mgx_summary_outputs* s, int i, double* p) {
  double** const arrays[NSLOTS - SLOT_LOUD] = {&s->loudness_specific, &s->mfcc, &s->amplitude_spectrum, &s->power_spectrum,
                                               NULL,                  NULL,     &s->mel_bands};
  if (i < MGX_NUM_SCALARS) s->scalars[i] = p;
  else if (arrays[i - SLOT_LOUD]) *arrays[i - SLOT_LOUD] = p;
}

/* Wanted outputs for j->nframes frames (a summary job: for j->nsignals signals). */
static int job_alloc(napi_env env, job* j, napi_value feats) {
  if (!parse_features(env, feats, j)) return 0;
  j->aux.struct_size = sizeof j->aux;
  for (int i = 0; i < NSLOTS; ++i) {
    if (!j->want[i]) continue;
    size_t b = (size_t)j->nframes * field_bytes(&j->box->desc, i);
    if (j->summary)
      b = (size_t)j->nsignals * MGX_NUM_STATS * sizeof(double) * (i < MGX_NUM_SCALARS ? 1 : field_bytes(&j->box->desc, i) / 4);
    j->bytes[i] = b;
    napi_value abv;
    void* data = NULL;
    if (napi_create_arraybuffer(env, b, &data, &abv) != napi_ok || napi_create_reference(env, abv, 1, &j->refs[i]) != napi_ok) {
      napi_throw_error(env, NULL, "out of host memory");
      return 0;
    }
    j->bufs[i] = data;
    if (j->summary) set_summary_field(&j->sum, i, (double*)data);
    else set_field(&j->out, &j->aux, i, data);
    /* the delta summaries of the same field: arrays of the same size (a spectrum's too: the library refuses it) */
    for (uint32_t k = 0; j->summary && k < j->delta_order; ++k) {
      if (napi_create_arraybuffer(env, b, &data, &abv) != napi_ok || napi_create_reference(env, abv, 1, &j->drefs[k][i]) != napi_ok) {
        napi_throw_error(env, NULL, "out of host memory");
        return 0;
      }
      set_summary_field(&j->dsum[k], i, (double*)data);
    }
  }
  return 1;
}

/* wavBytes: a Buffer / Uint8Array / ArrayBuffer holding a whole .wav file. */
static int bytes_of(napi_env env, napi_value v, const unsigned char** data, size_t* len) {
  bool is = false;
  void* d = NULL;
  napi_is_buffer(env, v, &is);
  if (is) {
    napi_get_buffer_info(env, v, &d, len);
    *data = (const unsigned char*)d;
    return 1;
  }
  napi_is_typedarray(env, v, &is);
  if (is) {
    napi_typedarray_type tt;
    size_t n = 0, off = 0;
    napi_value ab;
    napi_get_typedarray_info(env, v, &tt, &n, &d, &ab, &off);
    if (tt == napi_uint8_array || tt == napi_int8_array || tt == napi_uint8_clamped_array) {
      *data = (const unsigned char*)d;
      *len = n;
      return 1;
    }
  }
  napi_is_arraybuffer(env, v, &is);
  if (is) {
    napi_get_arraybuffer_info(env, v, &d, len);
    *data = (const unsigned char*)d;
    return 1;
  }
  napi_throw_type_error(env, NULL, "expected the bytes of a .wav file (Buffer, Uint8Array or ArrayBuffer)");
  return 0;
}

static int job_prepare_wav(napi_env env, job* j, napi_value wav_v, napi_value feats, napi_value chan_v, napi_value hop_v) {
  const unsigned char* data = NULL;
  size_t len = 0;
  if (!bytes_of(env, wav_v, &data, &len)) return 0;
  mgx_wav_info wi;
  memset(&wi, 0, sizeof wi);
  wi.struct_size = sizeof wi;
  int rc = mgx_wav_parse(data, len, &wi);
  if (rc) {
    throw_mgx(env, rc);
    return 0;
  }
  uint32_t ch = 0;
  if (chan_v) {
    napi_valuetype t;
    napi_typeof(env, chan_v, &t);
    if (t == napi_number) napi_get_value_uint32(env, chan_v, &ch);
  }
  if (ch >= wi.channels) {
    napi_throw_range_error(env, NULL, "channel out of range for this file");
    return 0;
  }
  j->pcm = data + wi.data_offset;
  j->pcm_bytes = wi.data_bytes;
  j->pcm_frames = wi.sample_frames;
  j->pcm_format = wi.pcm_format;
  j->pcm_channels = wi.channels;
  j->pcm_channel = ch;
  j->nframes = wi.sample_frames / j->box->desc.buffer_size;
  napi_valuetype ht = napi_undefined;
  if (hop_v) napi_typeof(env, hop_v, &ht);
  if (ht != napi_undefined) {  /* the trailing hop: the buffers that start every hop samples */
    if (!hop_of(env, j, hop_v, &j->hop)) return 0;
    rc = mgx_signal_frames(wi.sample_frames, j->box->desc.buffer_size, j->hop, &j->nframes);
    if (rc) {
      throw_mgx(env, rc);
      return 0;
    }
  }
  return job_alloc(env, j, feats);
}

static void job_run(job* j) {
  if (j->box->group && j->pcm) {
    j->rc = MGX_E_UNSUPPORTED;
    snprintf(j->err, sizeof j->err, "extractWav on a multi-device plan: use a single-device plan");
    return;
  }
  const uint32_t n = j->box->desc.buffer_size;
  if (j->hpss)
    j->rc = mgx_hpss_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals, &j->hpar,
                          j->hchroma ? &j->creq : NULL, j->hflux ? &j->flux[0] : NULL, j->hparts[0], j->hparts[1]);
  else if (j->chroma)
    j->rc = mgx_chroma_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals, &j->creq);
  else if (j->beats)
    j->rc = mgx_beats_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals, &j->flux[0],
                           &j->tpar, j->twindow, j->tprior, &j->bpar, j->bgauss, j->bpenalty, j->tlag, j->peak_offsets,
                           j->nframes ? j->peaks : NULL, j->nframes);
  else if (j->tempo)
    j->rc = mgx_tempo_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals, &j->flux[0],
                           &j->tpar, j->twindow, j->tprior, j->tsummary, j->tlag);
  else if (j->onsets)
    j->rc = mgx_onsets_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals, &j->flux[0],
                            &j->peak, j->peak_offsets, j->nframes ? j->peaks : NULL, j->nframes);
  else if (j->summary && j->num_flux)
    j->rc = mgx_summarize_flux_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals,
                                    NULL, NULL, &j->sum, j->delta_order ? &j->deltas : NULL, j->flux, j->num_flux);
  else if (j->summary && j->delta_order)
    j->rc = mgx_summarize_deltas_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals,
                                      NULL, NULL, &j->sum, &j->deltas);
  else if (j->summary)
    j->rc = mgx_summarize_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, j->frame_offsets, j->nsignals, NULL,
                               NULL, &j->sum);
  else if (j->gather)
    j->rc = mgx_extract_gather_host(j->box->plan, j->frames, j->nsamples, j->starts, j->nframes, &j->out,
                                    j->want[SLOT_MEL] ? &j->aux : NULL);
  else if (j->box->group)
    j->rc = mgx_group_extract_host(j->box->group, j->frames, j->nframes, &j->out);
  else if (j->want[SLOT_MEL] && j->pcm)  /* (a dense batch is the signal form at hop N) */
    j->rc = mgx_extract_host_pcm_ex(j->box->plan, j->pcm, j->pcm_bytes, j->pcm_frames, j->pcm_format, j->pcm_channels,
                                    j->pcm_channel, j->hop ? j->hop : n, &j->out, &j->aux);
  else if (j->want[SLOT_MEL])
    j->rc = mgx_extract_host_ex(j->box->plan, j->frames, j->hop ? j->nsamples : j->nframes * n, j->hop ? j->hop : n, &j->out,
                                &j->aux);
  else if (j->hop && j->pcm)
    j->rc = mgx_extract_signal_host_pcm(j->box->plan, j->pcm, j->pcm_bytes, j->pcm_frames, j->pcm_format, j->pcm_channels,
                                        j->pcm_channel, j->hop, &j->out);
  else if (j->hop)
    j->rc = mgx_extract_signal_host(j->box->plan, j->frames, j->nsamples, j->hop, &j->out);
  else if (j->pcm)
    j->rc = mgx_extract_host_pcm(j->box->plan, j->pcm, j->pcm_bytes, j->pcm_frames, j->pcm_format, j->pcm_channels,
                                 j->pcm_channel, &j->out);
  else
    j->rc = mgx_extract_host(j->box->plan, j->frames, j->nframes, &j->out);
  if (j->rc) snprintf(j->err, sizeof j->err, "%s", mgx_last_error());
}

static napi_value typed_of(napi_env env, napi_ref ref, size_t bytes, napi_typedarray_type t, size_t elem) {
  napi_value ab, ta;
  if (napi_get_reference_value(env, ref, &ab) != napi_ok) return NULL;
  if (napi_create_typedarray(env, t, bytes / elem, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}

static napi_value typed(napi_env env, job* j, int slot, napi_typedarray_type t, size_t elem) {
  return typed_of(env, j->refs[slot], j->bytes[slot], t, elem);
}

static napi_value job_result(napi_env env, job* j) {
  static const char* names[MGX_NUM_SCALARS] = {
      "rms", "energy", "zcr", "spectralCentroid", "spectralFlatness", "spectralSlope", "spectralRolloff",
      "spectralSpread", "spectralSkewness", "spectralKurtosis", "loudness.total", "perceptualSpread",
      "perceptualSharpness"};
  napi_value obj;
  if (napi_create_object(env, &obj) != napi_ok) return NULL;
  if (j->hpss) {
    const size_t cols = j->box->desc.buffer_size / 2, C = j->creq.num_chroma;
    static const char* const part[2] = {"harmonic", "percussive"};
    for (int i = 0; i < 2; ++i)
      if (j->hrefs[i])
        napi_set_named_property(env, obj, part[i], typed_of(env, j->hrefs[i], (size_t)j->nframes * cols * sizeof(float), napi_float32_array, 4));
    if (j->hchroma) {
      napi_value nc;
      if (napi_create_uint32(env, (uint32_t)C, &nc) != napi_ok) return NULL;
      napi_set_named_property(env, obj, "numChroma", nc);
      if (j->crefs[1])
        napi_set_named_property(env, obj, "chroma", typed_of(env, j->crefs[1], (size_t)j->nframes * C * sizeof(float), napi_float32_array, 4));
      if (j->crefs[2])
        napi_set_named_property(env, obj, "chromaSummary",
                                typed_of(env, j->crefs[2], (size_t)j->nsignals * MGX_NUM_STATS * C * sizeof(double), napi_float64_array, 8));
    }
    if (j->frefs[1][0])
      napi_set_named_property(env, obj, "flux", typed_of(env, j->frefs[1][0], (size_t)j->nframes * sizeof(float), napi_float32_array, 4));
    if (j->frefs[0][0])
      napi_set_named_property(env, obj, "fluxSummary",
                              typed_of(env, j->frefs[0][0], (size_t)j->nsignals * MGX_NUM_STATS * sizeof(double), napi_float64_array, 8));
    return obj;
  }
  if (j->chroma) {
    napi_value nc;
    const size_t C = j->creq.num_chroma;
    napi_set_named_property(env, obj, "chroma", typed_of(env, j->crefs[1], (size_t)j->nframes * C * sizeof(float), napi_float32_array, 4));
    if (napi_create_uint32(env, (uint32_t)C, &nc) != napi_ok) return NULL;
    napi_set_named_property(env, obj, "numChroma", nc);
    if (j->crefs[2])
      napi_set_named_property(env, obj, "summary",
                              typed_of(env, j->crefs[2], (size_t)j->nsignals * MGX_NUM_STATS * C * sizeof(double), napi_float64_array, 8));
    return obj;
  }
  if (j->tempo) {
    napi_value nl;
    const size_t L = j->tpar.num_lags;
    napi_set_named_property(env, obj, "lag", typed_of(env, j->trefs[2], (size_t)j->nsignals * sizeof(uint32_t), napi_uint32_array, 4));
    if (napi_create_uint32(env, (uint32_t)L, &nl) != napi_ok) return NULL;
    napi_set_named_property(env, obj, "numLags", nl);
    if (j->trefs[3])
      napi_set_named_property(env, obj, "summary",
                              typed_of(env, j->trefs[3], (size_t)j->nsignals * MGX_NUM_STATS * L * sizeof(double), napi_float64_array, 8));
    if (j->beats) {  /* the index arrays as onsetsGather returns its own: Float64Arrays */
      const uint64_t total = j->peak_offsets[j->nsignals];
      const uint64_t* const src[2] = {j->peak_offsets, j->peaks};
      const uint64_t count[2] = {j->nsignals + 1, total};
      static const char* const nm[2] = {"beatOffsets", "beats"};
      for (int k = 0; k < 2; ++k) {
        napi_value abv, ta;
        void* data = NULL;
        if (napi_create_arraybuffer(env, (size_t)count[k] * sizeof(double), &data, &abv) != napi_ok ||
            napi_create_typedarray(env, napi_float64_array, (size_t)count[k], abv, 0, &ta) != napi_ok)
          return NULL;
        for (uint64_t i = 0; i < count[k]; ++i) ((double*)data)[i] = (double)src[k][i];
        napi_set_named_property(env, obj, nm[k], ta);
      }
    }
    if (j->frefs[1][0])
      napi_set_named_property(env, obj, "envelope", typed_of(env, j->frefs[1][0], (size_t)j->nframes * sizeof(float), napi_float32_array, 4));
    return obj;
  }
  if (j->onsets) {  /* the index arrays as signalsFrameStarts returns its own: Float64Arrays */
    const uint64_t total = j->peak_offsets[j->nsignals];
    const uint64_t* const src[2] = {j->peak_offsets, j->peaks};
    const uint64_t count[2] = {j->nsignals + 1, total};
    static const char* const nm[2] = {"onsetOffsets", "onsets"};
    for (int k = 0; k < 2; ++k) {
      napi_value abv, ta;
      void* data = NULL;
      if (napi_create_arraybuffer(env, (size_t)count[k] * sizeof(double), &data, &abv) != napi_ok ||
          napi_create_typedarray(env, napi_float64_array, (size_t)count[k], abv, 0, &ta) != napi_ok)
        return NULL;
      for (uint64_t i = 0; i < count[k]; ++i) ((double*)data)[i] = (double)src[k][i];
      napi_set_named_property(env, obj, nm[k], ta);
    }
    if (j->frefs[1][0])
      napi_set_named_property(env, obj, "envelope", typed_of(env, j->frefs[1][0], (size_t)j->nframes * sizeof(float), napi_float32_array, 4));
    return obj;
  }
  if (j->summary) {  /* every summary is float64: the same names, each nsignals x 4 x width */
    static const char* arrays[NSLOTS - SLOT_LOUD] = {"loudness.specific", "mfcc", "amplitudeSpectrum", "powerSpectrum", NULL, NULL, "melBands"};
    for (int i = 0; i < NSLOTS; ++i) {
      const char* nm = i < MGX_NUM_SCALARS ? names[i] : arrays[i - SLOT_LOUD];
      if (j->want[i] && nm) napi_set_named_property(env, obj, nm, typed(env, j, i, napi_float64_array, 8));
    }
    /* the delta summaries: objects of the same names under "delta" and (order 2) "delta2" */
    for (uint32_t k = 0; k < j->delta_order; ++k) {
      napi_value sub;
      if (napi_create_object(env, &sub) != napi_ok) return NULL;
      for (int i = 0; i < NSLOTS; ++i) {
        const char* nm = i < MGX_NUM_SCALARS ? names[i] : arrays[i - SLOT_LOUD];
        if (j->want[i] && nm) napi_set_named_property(env, sub, nm, typed_of(env, j->drefs[k][i], j->bytes[i], napi_float64_array, 8));
      }
      napi_set_named_property(env, obj, k ? "delta2" : "delta", sub);
    }
    /* the flux: an array, one {summary, perFrame} per request */
    if (j->num_flux) {
      napi_value arr;
      if (napi_create_array_with_length(env, j->num_flux, &arr) != napi_ok) return NULL;
      for (uint32_t i = 0; i < j->num_flux; ++i) {
        napi_value one;
        if (napi_create_object(env, &one) != napi_ok) return NULL;
        if (j->frefs[0][i])
          napi_set_named_property(env, one, "summary",
                                  typed_of(env, j->frefs[0][i], (size_t)j->nsignals * MGX_NUM_STATS * sizeof(double), napi_float64_array, 8));
        if (j->frefs[1][i])
          napi_set_named_property(env, one, "perFrame", typed_of(env, j->frefs[1][i], (size_t)j->nframes * sizeof(float), napi_float32_array, 4));
        napi_set_element(env, arr, i, one);
      }
      napi_set_named_property(env, obj, "flux", arr);
    }
    return obj;
  }
  const int f64 = j->box->desc.scalar_f64;
  for (int i = 0; i < MGX_NUM_SCALARS; ++i)
    if (j->want[i]) napi_set_named_property(env, obj, names[i], typed(env, j, i, f64 ? napi_float64_array : napi_float32_array, f64 ? 8 : 4));
  if (j->want[SLOT_LOUD]) napi_set_named_property(env, obj, "loudness.specific", typed(env, j, SLOT_LOUD, napi_float32_array, 4));
  if (j->want[SLOT_MFCC]) napi_set_named_property(env, obj, "mfcc", typed(env, j, SLOT_MFCC, napi_float32_array, 4));
  if (j->want[SLOT_MEL]) napi_set_named_property(env, obj, "melBands", typed(env, j, SLOT_MEL, napi_float32_array, 4));
  if (j->want[SLOT_AMP]) napi_set_named_property(env, obj, "amplitudeSpectrum", typed(env, j, SLOT_AMP, napi_float32_array, 4));
  if (j->want[SLOT_POW]) napi_set_named_property(env, obj, "powerSpectrum", typed(env, j, SLOT_POW, napi_float32_array, 4));
  if (j->want[SLOT_CRE]) napi_set_named_property(env, obj, "complexSpectrum.real", typed(env, j, SLOT_CRE, napi_float32_array, 4));
  if (j->want[SLOT_CIM]) napi_set_named_property(env, obj, "complexSpectrum.imag", typed(env, j, SLOT_CIM, napi_float32_array, 4));
  return obj;
}

/* kind: the input of an extraction job */
enum { IN_FRAMES = 0, IN_WAV = 1, IN_SIGNAL = 2, IN_GATHER = 3, IN_SUMMARY = 4, IN_ONSETS = 5, IN_CHROMA = 6, IN_TEMPO = 7, IN_BEATS = 8, IN_HPSS = 9 };

static int job_prepare_kind(napi_env env, job* j, int kind, size_t argc, napi_value* argv) {
  if (kind == IN_WAV) return job_prepare_wav(env, j, argv[1], argv[2], argc > 3 ? argv[3] : NULL, argc > 4 ? argv[4] : NULL);
  if (kind == IN_SIGNAL) return job_prepare_signal(env, j, argv[1], argv[2], argv[3]);
  if (kind == IN_GATHER) return job_prepare_gather(env, j, argv[1], argv[2], argv[3]);
  if (kind == IN_SUMMARY) return job_prepare_summary(env, j, argv[1], argv[2], argv[3], argv[4], argc > 5 ? argv[5] : NULL);
  if (kind == IN_ONSETS) return job_prepare_onsets(env, j, argv[1], argv[2], argv[3], argv[4]);
  if (kind == IN_CHROMA) return job_prepare_chroma(env, j, argv[1], argv[2], argv[3], argv[4]);
  if (kind == IN_HPSS) return job_prepare_hpss(env, j, argv[1], argv[2], argv[3], argv[4]);
  if (kind == IN_TEMPO || kind == IN_BEATS) return job_prepare_tempo(env, j, argv[1], argv[2], argv[3], argv[4], kind == IN_BEATS);
  return job_prepare(env, j, argv[1], argv[2]);
}

static napi_value extract_common(napi_env env, napi_callback_info info, int kind) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < (kind == IN_SUMMARY || kind == IN_ONSETS || kind == IN_CHROMA || kind == IN_TEMPO || kind == IN_BEATS || kind == IN_HPSS ? 5u : kind == IN_SIGNAL || kind == IN_GATHER ? 4u : 3u)) {
    napi_throw_type_error(env, NULL, kind == IN_WAV ? "extractWav(plan, wavBytes, features[, channel[, hop]])"
                                   : kind == IN_HPSS ? "hpssGather(plan, samples, starts, frameOffsets, {kernelTime, kernelFreq, mode, ...})"
                                   : kind == IN_CHROMA ? "chromaGather(plan, samples, starts, frameOffsets, {weights, numChroma, ...})"
                                   : kind == IN_TEMPO ? "tempoGather(plan, samples, starts, frameOffsets, {field, window, prior, ...})"
                                   : kind == IN_BEATS ? "beatsGather(plan, samples, starts, frameOffsets, {field, window, prior, gauss, penalty, ...})"
                                   : kind == IN_ONSETS ? "onsetsGather(plan, samples, starts, frameOffsets, {field, ...})"
                                   : kind == IN_SUMMARY ? "summarizeGather(plan, samples, starts, frameOffsets, features[, {deltaWidth, deltaOrder}])"
                                   : kind == IN_GATHER ? "extractGather(plan, samples, starts, features)"
                                   : kind == IN_SIGNAL ? "extractSignal(plan, samples, hop, features)"
                                                       : "extract(plan, frames, features)");
    return NULL;
  }
  job j;
  memset(&j, 0, sizeof j);
  j.box = get_plan(env, argv[0]);
  if (!j.box) return NULL;
  if (j.box->busy) {
    napi_throw_error(env, NULL, "plan is busy with an async extraction");
    return NULL;
  }
  if (!job_prepare_kind(env, &j, kind, argc, argv)) {
    job_free_buffers(env, &j);
    return NULL;
  }
  job_run(&j);
  if (j.rc) {
    job_free_buffers(env, &j);
    char code[16];
    snprintf(code, sizeof code, "%d", j.rc);
    napi_throw_error(env, code, j.err);
    return NULL;
  }
  napi_value r = job_result(env, &j);
  job_free_buffers(env, &j);
  return r;
}

/* extractInto(plan, frames, offsets, out): the same synchronous extraction into ONE caller-provided
 * ArrayBuffer. offsets: a Float64Array of the 19 output fields' byte offsets in `out` (mgx_outputs
 * order: the 13 scalars, loudness_specific, mfcc, amplitude, power, complex real, complex imag; a
 * negative entry = not requested), or of 20: those, then melBands (mgx_aux_outputs.mel_bands). The facade's real-time paths (get(), batched streaming) lay the
 * outputs of a feature list out once and call this per buffer or batch: one allocation and a handful of
 * N-API calls instead of an ArrayBuffer, a reference and a typed array per output. */
static napi_value extract_into(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 4) {
    napi_throw_type_error(env, NULL, "extractInto(plan, frames, offsets, out)");
    return NULL;
  }
  plan_box* box = get_plan(env, argv[0]);
  if (!box) return NULL;
  if (box->busy) {
    napi_throw_error(env, NULL, "plan is busy with an async extraction");
    return NULL;
  }
  napi_typedarray_type tt;
  size_t len = 0, off = 0, olen = 0;
  void* data = NULL;
  void* offs = NULL;
  napi_value ab;
  bool is = false;
  napi_is_typedarray(env, argv[1], &is);
  if (is) napi_get_typedarray_info(env, argv[1], &tt, &len, &data, &ab, &off);
  if (!is || tt != napi_float32_array) {
    napi_throw_type_error(env, NULL, "frames must be a Float32Array");
    return NULL;
  }
  napi_is_typedarray(env, argv[2], &is);
  if (is) napi_get_typedarray_info(env, argv[2], &tt, &olen, &offs, &ab, &off);
  if (!is || tt != napi_float64_array || (olen != 19 && olen != 20)) {
    napi_throw_type_error(env, NULL, "offsets must be a Float64Array of 19 byte offsets (20 with melBands)");
    return NULL;
  }
  void* out = NULL;
  size_t out_bytes = 0;
  napi_is_arraybuffer(env, argv[3], &is);
  if (is) napi_get_arraybuffer_info(env, argv[3], &out, &out_bytes);
  if (!is) {
    napi_throw_type_error(env, NULL, "out must be an ArrayBuffer");
    return NULL;
  }
  const uint32_t n = box->desc.buffer_size;
  if (len % n) {
    napi_throw_range_error(env, NULL, "frames.length must be a multiple of bufferSize");
    return NULL;
  }
  const uint64_t F = len / n;
  const size_t ss = box->desc.scalar_f64 ? 8 : 4;
  void* ptr[NSLOTS];
  const double* o = (const double*)offs;
  for (int i = 0; i < NSLOTS; ++i) {
    ptr[i] = NULL;
    if (i >= (int)olen || !(o[i] >= 0)) continue;
    const double end = o[i] + (double)(field_bytes(&box->desc, i) * F);
    if (o[i] != (double)(uint64_t)o[i] || end > (double)out_bytes || ((uint64_t)o[i] % (i < MGX_NUM_SCALARS ? ss : 4))) {
      napi_throw_range_error(env, NULL, "an output's offset is misaligned or runs past the end of out");
      return NULL;
    }
    ptr[i] = (unsigned char*)out + (uint64_t)o[i];
  }
  if ((ptr[SLOT_CRE] == NULL) != (ptr[SLOT_CIM] == NULL)) {
    napi_throw_range_error(env, NULL, "complex real and imag go together");
    return NULL;
  }
  if (ptr[SLOT_MEL] && box->group) {
    napi_throw_error(env, NULL, "melBands is not supported on a plan created with `devices`: device groups take no auxiliary outputs");
    return NULL;
  }
  mgx_outputs mo;
  memset(&mo, 0, sizeof mo);
  mgx_aux_outputs ma;
  memset(&ma, 0, sizeof ma);
  ma.struct_size = sizeof ma;
  for (int i = 0; i < NSLOTS; ++i) set_field(&mo, &ma, i, ptr[i]);
  const int rc = box->group ? mgx_group_extract_host(box->group, (const float*)data, F, &mo)
                 : ptr[SLOT_MEL] ? mgx_extract_host_ex(box->plan, (const float*)data, F * n, n, &mo, &ma)
                            : mgx_extract_host(box->plan, (const float*)data, F, &mo);
  if (rc) return throw_mgx(env, rc);
  return argv[3];
}

static napi_value extract_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_FRAMES); }
static napi_value extract_wav_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_WAV); }
static napi_value extract_signal_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_SIGNAL); }
static napi_value extract_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_GATHER); }
static napi_value summarize_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_SUMMARY); }
static napi_value onsets_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_ONSETS); }
static napi_value chroma_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_CHROMA); }
static napi_value hpss_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_HPSS); }
static napi_value tempo_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_TEMPO); }
static napi_value beats_gather_sync(napi_env env, napi_callback_info info) { return extract_common(env, info, IN_BEATS); }

static void async_execute(napi_env env, void* data) {
  (void)env;
  job_run((job*)data);
}

static void async_complete(napi_env env, napi_status status, void* data) {
  job* j = (job*)data;
  plan_box* box = j->box;
  box->busy = 0;
  if (status != napi_ok || j->rc) {
    napi_value msg, err;
    napi_create_string_utf8(env, j->rc ? j->err : "async extraction cancelled", NAPI_AUTO_LENGTH, &msg);
    napi_create_error(env, NULL, msg, &err);
    napi_reject_deferred(env, j->deferred, err);
  } else {
    napi_resolve_deferred(env, j->deferred, job_result(env, j));
  }
  napi_delete_reference(env, j->frames_ref);
  napi_delete_reference(env, j->plan_ref);
  napi_delete_async_work(env, j->work);
  job_free_buffers(env, j);
  free(j);
  if (box->finalized) plan_box_free(box);
}

static napi_value extract_async_common(napi_env env, napi_callback_info info, int kind) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < (kind == IN_SUMMARY || kind == IN_ONSETS || kind == IN_CHROMA || kind == IN_TEMPO || kind == IN_BEATS || kind == IN_HPSS ? 5u : kind == IN_SIGNAL || kind == IN_GATHER ? 4u : 3u)) {
    napi_throw_type_error(env, NULL, kind == IN_WAV ? "extractWavAsync(plan, wavBytes, features[, channel[, hop]])"
                                   : kind == IN_HPSS ? "hpssGatherAsync(plan, samples, starts, frameOffsets, {kernelTime, kernelFreq, mode, ...})"
                                   : kind == IN_CHROMA ? "chromaGatherAsync(plan, samples, starts, frameOffsets, {weights, numChroma, ...})"
                                   : kind == IN_TEMPO ? "tempoGatherAsync(plan, samples, starts, frameOffsets, {field, window, prior, ...})"
                                   : kind == IN_BEATS ? "beatsGatherAsync(plan, samples, starts, frameOffsets, {field, window, prior, gauss, penalty, ...})"
                                   : kind == IN_ONSETS ? "onsetsGatherAsync(plan, samples, starts, frameOffsets, {field, ...})"
                                   : kind == IN_SUMMARY ? "summarizeGatherAsync(plan, samples, starts, frameOffsets, features[, {deltaWidth, deltaOrder}])"
                                   : kind == IN_GATHER ? "extractGatherAsync(plan, samples, starts, features)"
                                   : kind == IN_SIGNAL ? "extractSignalAsync(plan, samples, hop, features)"
                                                       : "extractAsync(plan, frames, features)");
    return NULL;
  }
  job* j = (job*)calloc(1, sizeof *j);
  j->box = get_plan(env, argv[0]);
  if (!j->box) { free(j); return NULL; }
  if (j->box->busy) {
    free(j);
    napi_throw_error(env, NULL, "plan is busy with an async extraction");
    return NULL;
  }
  if (!job_prepare_kind(env, j, kind, argc, argv)) {
    job_free_buffers(env, j);
    free(j);
    return NULL;
  }
  napi_value promise, name;
  CHECK(napi_create_reference(env, argv[1], 1, &j->frames_ref));  /* keep the input alive */
  CHECK(napi_create_reference(env, argv[0], 1, &j->plan_ref));    /* and the plan */
  CHECK(napi_create_promise(env, &j->deferred, &promise));
  CHECK(napi_create_string_utf8(env, "meyda_extract", NAPI_AUTO_LENGTH, &name));
  CHECK(napi_create_async_work(env, NULL, name, async_execute, async_complete, j, &j->work));
  j->box->busy = 1;
  CHECK(napi_queue_async_work(env, j->work));
  return promise;
}

static napi_value extract_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_FRAMES); }
static napi_value extract_wav_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_WAV); }
static napi_value extract_signal_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_SIGNAL); }
static napi_value extract_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_GATHER); }
static napi_value summarize_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_SUMMARY); }
static napi_value onsets_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_ONSETS); }
static napi_value chroma_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_CHROMA); }
static napi_value hpss_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_HPSS); }
static napi_value tempo_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_TEMPO); }
static napi_value beats_gather_async(napi_env env, napi_callback_info info) { return extract_async_common(env, info, IN_BEATS); }

/* chromaWeights(bufferSize, sampleRate[, {numChroma, a440, centerOctave, octaveWidth, baseC}]): the chroma filter
 * bank (mgx_chroma_weights; host only), a Float32Array of numChroma x bufferSize / 2, row-major. */
static napi_value chroma_weights(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double n = 0, sr = 0;
  napi_valuetype t0 = napi_undefined, t1 = napi_undefined, ot = napi_undefined;
  if (argc >= 2) napi_typeof(env, argv[0], &t0), napi_typeof(env, argv[1], &t1);
  if (t0 != napi_number || t1 != napi_number) {
    napi_throw_type_error(env, NULL, "chromaWeights(bufferSize, sampleRate[, {numChroma, a440, centerOctave, octaveWidth, baseC}])");
    return NULL;
  }
  napi_get_value_double(env, argv[0], &n);
  napi_get_value_double(env, argv[1], &sr);
  if (!(n >= 0) || n > 4294967295.0 || n != (double)(uint32_t)n) {
    napi_throw_range_error(env, NULL, "bufferSize must be a non-negative integer");
    return NULL;
  }
  mgx_chroma_params p;
  mgx_chroma_params_init(&p);
  if (argc > 2) napi_typeof(env, argv[2], &ot);
  if (ot == napi_object) {
    napi_value v;
    bool b = true;
    if (!option_u32(env, argv[2], "numChroma", 1, MGX_CHROMA_MAX_BINS, 12, &p.num_chroma)) return NULL;
    if (!option_f64(env, argv[2], "a440", &p.a440) || !option_f64(env, argv[2], "centerOctave", &p.center_octave) ||
        !option_f64(env, argv[2], "octaveWidth", &p.octave_width))
      return NULL;
    if (option_given(env, argv[2], "baseC", &v)) napi_coerce_to_bool(env, v, &v), napi_get_value_bool(env, v, &b);
    p.base_c = b ? 1 : 0;
  } else if (ot != napi_undefined && ot != napi_null) {
    napi_throw_type_error(env, NULL, "options must be an object: {numChroma, a440, centerOctave, octaveWidth, baseC}");
    return NULL;
  }
  /* (a size the library refuses may leave nothing to point at: it checks the size before it writes) */
  const int pow2 = (uint32_t)n >= 4 && ((uint32_t)n & ((uint32_t)n - 1)) == 0;
  const size_t count = pow2 ? (size_t)p.num_chroma * ((uint32_t)n / 2) : 1;
  napi_value ab, ta;
  void* data = NULL;
  CHECK(napi_create_arraybuffer(env, count * sizeof(float), &data, &ab));
  const int rc = mgx_chroma_weights((uint32_t)n, sr, &p, (float*)data);
  if (rc) return throw_mgx(env, rc);
  CHECK(napi_create_typedarray(env, napi_float32_array, count, ab, 0, &ta));
  return ta;
}

/* tempogramWindow(winLength): the periodic Hann window of the tempogram (mgx_tempogram_window; host only), a
 * Float32Array of winLength. */
static napi_value tempogram_window(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double w = 0;
  napi_valuetype t0 = napi_undefined;
  if (argc >= 1) napi_typeof(env, argv[0], &t0);
  if (t0 != napi_number) {
    napi_throw_type_error(env, NULL, "tempogramWindow(winLength)");
    return NULL;
  }
  napi_get_value_double(env, argv[0], &w);
  if (!(w >= 2) || w > MGX_TEMPOGRAM_MAX_WIN || w != (double)(uint32_t)w) {
    napi_throw_range_error(env, NULL, "winLength must be an integer from 2 to 1024");
    return NULL;
  }
  napi_value ab, ta;
  void* data = NULL;
  CHECK(napi_create_arraybuffer(env, (size_t)w * sizeof(float), &data, &ab));
  const int rc = mgx_tempogram_window((uint32_t)w, (float*)data);
  if (rc) return throw_mgx(env, rc);
  CHECK(napi_create_typedarray(env, napi_float32_array, (size_t)w, ab, 0, &ta));
  return ta;
}

/* tempoPrior(frameRate, numLags[, {startBpm = 120, stdOctaves = 1, maxBpm = 320}]): the log-normal tempo prior over the
 * lags of an envelope of frameRate rows a second (mgx_tempo_prior; host only), a Float64Array of numLags. */
static napi_value tempo_prior(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double rate = 0, nl = 0, start = 120.0, std = 1.0, mx = 320.0;
  napi_valuetype t0 = napi_undefined, t1 = napi_undefined, ot = napi_undefined;
  if (argc >= 2) napi_typeof(env, argv[0], &t0), napi_typeof(env, argv[1], &t1);
  if (t0 != napi_number || t1 != napi_number) {
    napi_throw_type_error(env, NULL, "tempoPrior(frameRate, numLags[, {startBpm, stdOctaves, maxBpm}])");
    return NULL;
  }
  napi_get_value_double(env, argv[0], &rate);
  napi_get_value_double(env, argv[1], &nl);
  if (!(nl >= 1) || nl > MGX_TEMPOGRAM_MAX_WIN || nl != (double)(uint32_t)nl) {
    napi_throw_range_error(env, NULL, "numLags must be an integer from 1 to 1024");
    return NULL;
  }
  if (argc > 2) napi_typeof(env, argv[2], &ot);
  if (ot == napi_object) {
    if (!option_f64(env, argv[2], "startBpm", &start) || !option_f64(env, argv[2], "stdOctaves", &std) ||
        !option_f64(env, argv[2], "maxBpm", &mx))
      return NULL;
  } else if (ot != napi_undefined && ot != napi_null) {
    napi_throw_type_error(env, NULL, "options must be an object: {startBpm, stdOctaves, maxBpm}");
    return NULL;
  }
  napi_value ab, ta;
  void* data = NULL;
  CHECK(napi_create_arraybuffer(env, (size_t)nl * sizeof(double), &data, &ab));
  const int rc = mgx_tempo_prior(rate, start, std, mx, (uint32_t)nl, (double*)data);
  if (rc) return throw_mgx(env, rc);
  CHECK(napi_create_typedarray(env, napi_float64_array, (size_t)nl, ab, 0, &ta));
  return ta;
}

/* beatTables(maxPeriod[, tightness = 100]): the tables of the beat tracker for the periods 1 .. maxPeriod
 * (mgx_beat_tables; host only): {gauss: a Float32Array of (maxPeriod + 1)(maxPeriod + 2) / 2, penalty: a Float64Array of
 * (maxPeriod + 1)^2}. */
static napi_value beat_tables(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double p = 0, tight = 100.0;
  napi_valuetype t0 = napi_undefined, t1 = napi_undefined;
  if (argc >= 1) napi_typeof(env, argv[0], &t0);
  if (argc >= 2) napi_typeof(env, argv[1], &t1);
  if (t0 != napi_number || (t1 != napi_number && t1 != napi_undefined)) {
    napi_throw_type_error(env, NULL, "beatTables(maxPeriod[, tightness])");
    return NULL;
  }
  napi_get_value_double(env, argv[0], &p);
  if (t1 == napi_number) napi_get_value_double(env, argv[1], &tight);
  if (!(p >= 1) || p > MGX_BEAT_MAX_PERIOD || p != (double)(uint32_t)p) {
    napi_throw_range_error(env, NULL, "maxPeriod must be an integer from 1 to 1023");
    return NULL;
  }
  const size_t P = (size_t)p, ng = (P + 1) * (P + 2) / 2, np = (P + 1) * (P + 1);
  napi_value gab, pab, gta, pta, obj;
  void *gdata = NULL, *pdata = NULL;
  CHECK(napi_create_arraybuffer(env, ng * sizeof(float), &gdata, &gab));
  CHECK(napi_create_arraybuffer(env, np * sizeof(double), &pdata, &pab));
  const int rc = mgx_beat_tables((uint32_t)P, tight, (float*)gdata, (double*)pdata);
  if (rc) return throw_mgx(env, rc);
  CHECK(napi_create_typedarray(env, napi_float32_array, ng, gab, 0, &gta));
  CHECK(napi_create_typedarray(env, napi_float64_array, np, pab, 0, &pta));
  CHECK(napi_create_object(env, &obj));
  CHECK(napi_set_named_property(env, obj, "gauss", gta));
  CHECK(napi_set_named_property(env, obj, "penalty", pta));
  return obj;
}

/* signalsFrameStarts(lengths, bufferSize, hop): mgx_signals_frame_starts (host only) for signals stored one after
 * another; lengths: a Float64Array. Returns {starts, frameOffsets}, Float64Arrays. */
static napi_value signals_frame_starts(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "signalsFrameStarts(lengths, bufferSize, hop)");
    return NULL;
  }
  double v[2] = {0, 0};
  for (int i = 0; i < 2; ++i) {
    napi_valuetype t = napi_undefined;
    napi_typeof(env, argv[1 + i], &t);
    if (t == napi_number) napi_get_value_double(env, argv[1 + i], &v[i]);
    if (t != napi_number || !(v[i] >= 0) || v[i] > 4294967295.0 || v[i] != (double)(uint64_t)v[i]) {
      napi_throw_range_error(env, NULL, "signalsFrameStarts(lengths, bufferSize, hop): non-negative integers");
      return NULL;
    }
  }
  size_t ns = 0;
  uint64_t* len = u64_of_f64(env, argv[0], "lengths", &ns);
  if (!len) return NULL;
  uint64_t* off = (uint64_t*)malloc((ns + 1) * sizeof *off);
  uint64_t* fo = (uint64_t*)malloc((ns + 1) * sizeof *fo);
  uint64_t* st = NULL;
  uint64_t total = 0;
  napi_value r = NULL;
  int rc = off && fo ? MGX_OK : MGX_E_OUT_OF_MEMORY;
  if (!rc) {
    off[0] = 0;
    for (size_t i = 0; i < ns; ++i) {
      /* (each length is below 2^53; their sum has to stay a sample index JavaScript can hold) */
      if (len[i] > 9007199254740991ull - off[i]) {
        char msg[96];
        snprintf(msg, sizeof msg, "lengths[0..%zu] add up to more than a safe integer", i);
        free(len);
        free(off);
        free(fo);
        napi_throw_range_error(env, NULL, msg);
        return NULL;
      }
      off[i + 1] = off[i] + len[i];
    }
    rc = mgx_signals_frame_starts(off, ns, (uint32_t)v[0], (uint32_t)v[1], NULL, NULL, 0, &total);
  }
  if (!rc) {
    st = (uint64_t*)malloc((total ? total : 1) * sizeof *st);
    rc = st ? mgx_signals_frame_starts(off, ns, (uint32_t)v[0], (uint32_t)v[1], fo, st, total, &total) : MGX_E_OUT_OF_MEMORY;
  }
  if (rc == MGX_E_OUT_OF_MEMORY) {
    napi_throw_error(env, NULL, "out of host memory");
  } else if (rc) {
    throw_mgx(env, rc);
  } else {
    napi_value ab, ta, obj;
    void* d = NULL;
    if (napi_create_object(env, &obj) == napi_ok && napi_create_arraybuffer(env, total * 8, &d, &ab) == napi_ok &&
        napi_create_typedarray(env, napi_float64_array, total, ab, 0, &ta) == napi_ok) {
      for (uint64_t i = 0; i < total; ++i) ((double*)d)[i] = (double)st[i];
      napi_set_named_property(env, obj, "starts", ta);
      if (napi_create_arraybuffer(env, (ns + 1) * 8, &d, &ab) == napi_ok &&
          napi_create_typedarray(env, napi_float64_array, ns + 1, ab, 0, &ta) == napi_ok) {
        for (size_t i = 0; i <= ns; ++i) ((double*)d)[i] = (double)fo[i];
        napi_set_named_property(env, obj, "frameOffsets", ta);
        r = obj;
      }
    }
    if (!r) napi_throw_error(env, NULL, "out of host memory");
  }
  free(len);
  free(off);
  free(fo);
  free(st);
  return r;
}

/* signalFrames(numSamples, bufferSize, hop): mgx_signal_frames (host only). */
static napi_value signal_frames(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], r;
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double v[3] = {0, 0, 0};
  for (size_t i = 0; i < 3; ++i) {
    napi_valuetype t = napi_undefined;
    if (i < argc) napi_typeof(env, argv[i], &t);
    if (t == napi_number) napi_get_value_double(env, argv[i], &v[i]);
    if (t != napi_number || !(v[i] >= 0) || v[i] > 9007199254740992.0 || v[i] != (double)(uint64_t)v[i] ||
        (i > 0 && v[i] > 4294967295.0)) {
      napi_throw_range_error(env, NULL, "signalFrames(numSamples, bufferSize, hop): non-negative integers");
      return NULL;
    }
  }
  uint64_t f = 0;
  int rc = mgx_signal_frames((uint64_t)v[0], (uint32_t)v[1], (uint32_t)v[2], &f);
  if (rc) return throw_mgx(env, rc);
  CHECK(napi_create_double(env, (double)f, &r));
  return r;
}

static napi_value wav_parse(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  const unsigned char* data = NULL;
  size_t len = 0;
  if (argc < 1 || !bytes_of(env, argv[0], &data, &len)) return NULL;
  mgx_wav_info wi;
  memset(&wi, 0, sizeof wi);
  wi.struct_size = sizeof wi;
  int rc = mgx_wav_parse(data, len, &wi);
  if (rc) return throw_mgx(env, rc);
  static const char* fmts[] = {"f32", "s16", "u8", "s24", "s32"};
  napi_value obj, v;
  CHECK(napi_create_object(env, &obj));
  CHECK(napi_create_string_utf8(env, fmts[wi.pcm_format], NAPI_AUTO_LENGTH, &v));
  CHECK(napi_set_named_property(env, obj, "pcmFormat", v));
  const struct { const char* k; double v; } nums[] = {
      {"channels", wi.channels}, {"sampleRate", wi.sample_rate}, {"bitsPerSample", wi.bits_per_sample},
      {"blockAlign", wi.block_align}, {"dataOffset", (double)wi.data_offset}, {"dataBytes", (double)wi.data_bytes},
      {"sampleFrames", (double)wi.sample_frames}};
  for (size_t i = 0; i < sizeof nums / sizeof nums[0]; ++i) {
    CHECK(napi_create_double(env, nums[i].v, &v));
    CHECK(napi_set_named_property(env, obj, nums[i].k, v));
  }
  return obj;
}

/* ---------------------------------------------------------------- host tables */
static napi_value host_tables(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  mgx_plan_desc d;
  if (argc) desc_from_opts(env, argv[0], &d);
  else mgx_plan_desc_init(&d);
  const size_t n = d.buffer_size, nf = d.num_mel_bands, nc = d.num_mfcc_coeffs;
  if (n > (1u << 20) || nf > 64 || nc > 64) {
    napi_throw_range_error(env, NULL, "hostTables: size out of range");
    return NULL;
  }
  napi_value ab[7];
  void* p[7];
  size_t sz[7] = {n * 4, n * 4, n * 4, n * 4, 25 * 4, (nf + 2) * 4, nc * nf * 4};
  for (int i = 0; i < 7; ++i) CHECK(napi_create_arraybuffer(env, sz[i], &p[i], &ab[i]));
  mgx_host_tables t = {(float*)p[0], (float*)p[1], (float*)p[2], (float*)p[3], (int32_t*)p[4], (int32_t*)p[5], (float*)p[6]};
  int rc = mgx_get_host_tables(&d, &t);
  if (rc) return throw_mgx(env, rc);
  static const char* keys[7] = {"window", "hanning", "hamming", "barkScale", "barkLimits", "melBins", "dct"};
  napi_value obj;
  CHECK(napi_create_object(env, &obj));
  for (int i = 0; i < 7; ++i) {
    napi_value ta;
    const int is_int = (i == 4 || i == 5);
    CHECK(napi_create_typedarray(env, is_int ? napi_int32_array : napi_float32_array, sz[i] / 4, ab[i], 0, &ta));
    CHECK(napi_set_named_property(env, obj, keys[i], ta));
  }
  return obj;
}

static napi_value is_pow2(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], r;
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  double v = 0;
  napi_valuetype t = napi_undefined;
  if (argc) napi_typeof(env, argv[0], &t);
  if (t == napi_number) napi_get_value_double(env, argv[0], &v);
  else v = 0; /* undefined % 2 is NaN in JS: not a power of two */
  CHECK(napi_get_boolean(env, t == napi_number && mgx_is_power_of_two(v), &r));
  return r;
}

static napi_value device_count(napi_env env, napi_callback_info info) {
  (void)info;
  int c = 0;
  mgx_device_count(&c);
  napi_value r;
  CHECK(napi_create_int32(env, c, &r));
  return r;
}

static napi_value feature_names(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value arr;
  CHECK(napi_create_array(env, &arr));
  for (int i = 0; i < MGX_NUM_FEATURES; ++i) {
    napi_value s;
    CHECK(napi_create_string_utf8(env, mgx_feature_name(i), NAPI_AUTO_LENGTH, &s));
    CHECK(napi_set_element(env, arr, i, s));
  }
  return arr;
}

static napi_value feature_info(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], r;
  CHECK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  char name[64] = {0};
  size_t len = 0;
  if (argc) napi_get_value_string_utf8(env, argv[0], name, sizeof name, &len);
  CHECK(napi_create_int32(env, mgx_feature_info(mgx_feature_index(name)), &r));
  return r;
}

static napi_value abi_version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  CHECK(napi_create_int32(env, mgx_abi_version(), &r));
  return r;
}

static napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"createPlan", NULL, create_plan, NULL, NULL, NULL, napi_enumerable, NULL},
      {"destroyPlan", NULL, destroy_plan, NULL, NULL, NULL, napi_enumerable, NULL},
      {"planBusy", NULL, plan_busy, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extract", NULL, extract_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractInto", NULL, extract_into, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractAsync", NULL, extract_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractWav", NULL, extract_wav_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractWavAsync", NULL, extract_wav_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractSignal", NULL, extract_signal_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractSignalAsync", NULL, extract_signal_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"signalFrames", NULL, signal_frames, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractGather", NULL, extract_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"extractGatherAsync", NULL, extract_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"summarizeGather", NULL, summarize_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"summarizeGatherAsync", NULL, summarize_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"onsetsGather", NULL, onsets_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"onsetsGatherAsync", NULL, onsets_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"chromaGather", NULL, chroma_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"chromaGatherAsync", NULL, chroma_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"chromaWeights", NULL, chroma_weights, NULL, NULL, NULL, napi_enumerable, NULL},
      {"hpssGather", NULL, hpss_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"hpssGatherAsync", NULL, hpss_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"tempoGather", NULL, tempo_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"tempoGatherAsync", NULL, tempo_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"tempogramWindow", NULL, tempogram_window, NULL, NULL, NULL, napi_enumerable, NULL},
      {"tempoPrior", NULL, tempo_prior, NULL, NULL, NULL, napi_enumerable, NULL},
      {"beatsGather", NULL, beats_gather_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"beatsGatherAsync", NULL, beats_gather_async, NULL, NULL, NULL, napi_enumerable, NULL},
      {"beatTables", NULL, beat_tables, NULL, NULL, NULL, napi_enumerable, NULL},
      {"signalsFrameStarts", NULL, signals_frame_starts, NULL, NULL, NULL, napi_enumerable, NULL},
      {"wavParse", NULL, wav_parse, NULL, NULL, NULL, napi_enumerable, NULL},
      {"hostTables", NULL, host_tables, NULL, NULL, NULL, napi_enumerable, NULL},
      {"isPowerOfTwo", NULL, is_pow2, NULL, NULL, NULL, napi_enumerable, NULL},
      {"deviceCount", NULL, device_count, NULL, NULL, NULL, napi_enumerable, NULL},
      {"featureNames", NULL, feature_names, NULL, NULL, NULL, napi_enumerable, NULL},
      {"featureInfo", NULL, feature_info, NULL, NULL, NULL, napi_enumerable, NULL},
      {"abiVersion", NULL, abi_version, NULL, NULL, NULL, napi_enumerable, NULL},
  };
  if (napi_define_properties(env, exports, sizeof props / sizeof props[0], props) != napi_ok) return NULL;
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
