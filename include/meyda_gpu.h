/*
 * meyda_gpu.h — C ABI of the MI355X (gfx950) meyda feature-extraction engine.
 *
 * This is the drop-in boundary for the reference's per-buffer hot path. In the
 * reference (kirbysayshi/meyda), one call of the path is:
 *
 *   src/meyda.js:69-91    onaudioprocess: window -> (FFT) -> amplitude spectrum
 *   src/meyda.js:244-261  Meyda.get(feature | features[]) -> extractor modules
 *   src/extractors/NAME.js  the 18 extractor plugins, signature (bufferSize, m)
 *
 * The engine batches that path: many frames of `buffer_size` Float32 samples are
 * processed by one fused HIP launch. A host binding (the N-API addon under
 * meyda_amd/addon/, or ctypes) maps Meyda's get()/start()/stop() onto it.
 *
 * Entry points and the reference interface each one replaces:
 *   mgx_plan_create      new Meyda(audioContext, src, bufferSize)   src/meyda.js:17-97
 *                        (power-of-two check src/meyda.js:20-22, tables :44-48,
 *                         extractor init :208-225)
 *   mgx_extract_device   onaudioprocess + get(features)             src/meyda.js:69-91,244-261
 *   mgx_extract_host     same, for host (pageable) buffers
 *   mgx_wav_parse,       decodeAudioData + getChannelData(0)        lib/bufferLoader.js:23,
 *   mgx_pcm_decode_device,                                          src/meyda.js:72
 *   mgx_extract_host_pcm
 *   mgx_extract_signal_* the same over one contiguous signal whose   src/meyda.js:69-91 (disjoint
 *                        buffers start every `hop` samples           buffers only: hop = N)
 *   mgx_extract_*_ex     the signal calls with the outputs added     src/extractors/mfcc.js:53-65
 *                        after mgx_outputs (mgx_aux_outputs):       (loggedMelBands, the Float32Array
 *                        melBands, the log mel band energies        the DCT of :67-93 reads)
 *   mgx_extract_gather_* the same over buffers that start where a    src/meyda.js:69-91 (one source,
 *   mgx_signals_frame_starts  table says: every buffer of every     one buffer per call)
 *                        clip of a corpus in one launch
 *   mgx_summarize_*      the gather calls with every clip's rows     no counterpart, as with the groups:
 *                        pooled on the device: mean, variance, min   the per-clip pooling loop of a host
 *                        and max of each output over a clip          application over Meyda.get's results
 *   mgx_delta_device,    the rows' time derivatives (delta, delta-  no counterpart: the regression
 *   mgx_summarize_deltas_*  delta) per frame, and pooled per clip    stencil of a host application
 *   mgx_flux_device,     spectral flux: the distance of a row from   no counterpart in this snapshot (one
 *   mgx_summarize_flux_*  an earlier row of its clip, per frame     buffer per call); later Meyda's
 *                        (the onset envelope) and pooled per clip    spectralFlux, Dixon's rectified flux
 *   mgx_peaks_device,    onsets: the peaks of a clip's envelope,     no counterpart: librosa.util.peak_pick
 *   mgx_onsets_host      picked on the device                        in a host application
 *   mgx_chroma_weights,  chroma: the pitch-class profile of every    no counterpart in this snapshot; later
 *   mgx_chroma_device,   amplitude row (a dense C x N/2 filter       Meyda's chroma (createChromaFilterBank,
 *   mgx_chroma_host      bank), per frame and pooled per clip        librosa.filters.chroma)
 *   mgx_tempogram_device, tempo: the local autocorrelation of a       no counterpart: librosa.feature.tempogram
 *   mgx_tempo_device,    clip's envelope per frame, pooled per clip,  and librosa.feature.tempo in a host
 *   mgx_tempo_host       and the lag a tempo prior picks              application
 *   mgx_beat_tables,     beats: a clip's beats placed on its         no counterpart: librosa.beat.beat_track's
 *   mgx_beats_device,    envelope at the tempo's lag by dynamic      tracker in a host application
 *   mgx_beats_host       programming
 *   mgx_group_*          several devices, RCCL gather of the        src/meyda.js:17-97 (one plan
 *                        per-frame records to the root device       per device), :69-91 (buffers
 *                                                                   are independent: shardable)
 *   mgx_feature_index    the extractor registry by name             src/extractors/index.js:1-20
 *   mgx_feature_info     featureInfo[name].type                     src/feature-info.js:1-65
 *   mgx_last_error       console.error / thrown Error text          src/meyda.js:20-26,249-253
 *
 * Conventions: every function returns an int status (MGX_OK = 0, negative =
 * MGX_E_*); the message of the last failure on the calling thread is returned
 * by mgx_last_error(). Plans are not thread-safe; distinct plans are
 * independent. No torch or HIP types appear in these signatures: streams are
 * passed as `void*` (a hipStream_t, or NULL for the default stream).
 */
#ifndef MEYDA_GPU_H
#define MEYDA_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGX_ABI_VERSION 2  /* 2: mgx_extract_host_pcm takes the PCM byte count; mgx_plan_desc.flags;
                              multi-device groups */

typedef enum mgx_status {
  MGX_OK = 0,
  MGX_E_INVALID_ARGUMENT = -1,   /* NULL pointer, bad enum, bad struct_size */
  MGX_E_NOT_POWER_OF_TWO = -2,   /* "Buffer size is not a power of two" (src/meyda.js:20-22) */
  MGX_E_UNSUPPORTED = -3,        /* valid request this build does not implement */
  MGX_E_DEVICE = -4,             /* a HIP runtime call failed */
  MGX_E_OUT_OF_MEMORY = -5,
  MGX_E_NO_DEVICE = -6           /* no usable gfx950 device */
} mgx_status;

/* Feature indices. The first 13 are the per-frame scalar record, in this order. */
typedef enum mgx_feature {
  MGX_RMS = 0,                  /* src/extractors/rms.js */
  MGX_ENERGY = 1,               /* energy.js */
  MGX_ZCR = 2,                  /* zcr.js (exact integer count) */
  MGX_SPECTRAL_CENTROID = 3,    /* spectralCentroid.js (bin units, as the reference) */
  MGX_SPECTRAL_FLATNESS = 4,    /* spectralFlatness.js */
  MGX_SPECTRAL_SLOPE = 5,       /* spectralSlope.js */
  MGX_SPECTRAL_ROLLOFF = 6,     /* spectralRolloff.js (Hz) */
  MGX_SPECTRAL_SPREAD = 7,      /* spectralSpread.js */
  MGX_SPECTRAL_SKEWNESS = 8,    /* spectralSkewness.js */
  MGX_SPECTRAL_KURTOSIS = 9,    /* spectralKurtosis.js */
  MGX_LOUDNESS_TOTAL = 10,      /* loudness.js .total */
  MGX_PERCEPTUAL_SPREAD = 11,   /* perceptualSpread.js */
  MGX_PERCEPTUAL_SHARPNESS = 12,/* perceptualSharpness.js */
  MGX_NUM_SCALARS = 13,
  /* vector features (pointer fields of mgx_outputs) */
  MGX_LOUDNESS = 13,            /* loudness.js: {specific: Float32Array(24), total} */
  MGX_MFCC = 14,                /* mfcc.js: Float32Array(13) */
  MGX_AMPLITUDE_SPECTRUM = 15,  /* amplitudeSpectrum.js */
  MGX_POWER_SPECTRUM = 16,      /* powerSpectrum.js */
  MGX_COMPLEX_SPECTRUM = 17,    /* complexSpectrum.js: {real, imag} */
  MGX_BUFFER = 18,              /* buffer (declared in feature-info.js:3-5): the frame itself */
  MGX_MEL_BANDS = 19,           /* mfcc.js:53-65 loggedMelBands: Float32Array(num_mel_bands), the log mel band
                                   energies the MFCC is the DCT of (melBands in later Meyda releases); a
                                   field of mgx_aux_outputs, not of mgx_outputs */
  MGX_NUM_FEATURES = 20
} mgx_feature;

typedef enum mgx_window { MGX_WINDOW_HANNING = 0, MGX_WINDOW_HAMMING = 1 } mgx_window;

typedef enum mgx_precision {
  /* FP64 butterflies, every radix-2 stage rounded to float32 as jsfft stores it
   * (lib/jsfft/fft.js:153-161 + Float32Array storage). Parity default. */
  MGX_PRECISION_FAITHFUL = 0,
  /* float32 butterflies, float32 twiddles, float32 amplitude sqrtf(re^2 + im^2): HBM-bound. What it promises
   * (tests/test_gpu_fast.py holds every buffer size and route to it; measured in profiles/fast_precision.txt):
   *  - amplitudeSpectrum and complexSpectrum lie within (7 log2 N + 2) 2^-24 of the exact transform of the
   *    windowed frame, X = fft(float32(x w)) / sqrt(N), in relative 2-norm per frame (3.5e-6 at N = 256,
   *    5.1e-6 at N = 4096: the bound of a float32 radix-2 FFT; measured 0.05-0.08 of it), and the amplitudes
   *    within 1e-5 ||ref||_inf of the reference's; powerSpectrum is the float32 square of the amplitudes;
   *  - every feature behind the spectrum is the reference's feature of THAT spectrum within 1e-5; rms, energy
   *    and zcr are the faithful precision's bits.
   * What it does not promise: the reference's own value of a feature that takes the logarithm of small bins
   * or bands (spectralFlatness, mfcc, melBands, loudness) on tonal, steep or impulsive frames. The spectrum's
   * error is absolute in the frame's norm, about 3e-7 ||X||, so a bin that far below the frame's largest has
   * no correct digit left: profiles/fast_precision.txt lists the deviation per feature and kind of frame.
   * Magnitude range: a bin with |X| >= 2^64 is returned as Inf, one below 2^-63 with a few significant bits,
   * one below 2^-75 as 0 (the squares are float32), where the faithful precision returns every float32
   * amplitude; |X| <= sqrt(N) / 2 of the largest sample. Inside the range a frame scaled by 2^k gives the same
   * spectra scaled by 2^k, bit for bit. */
  MGX_PRECISION_FAST = 1
} mgx_precision;

typedef enum mgx_mode {
  MGX_MODE_PER_BUFFER_FFT = 0,  /* the intended path: FFT of every buffer */
  MGX_MODE_LITERAL = 1          /* the snapshot's behaviour: ampSpectrum = |window * x|,
                                   no per-buffer FFT (src/meyda.js:79-84,184-197) */
} mgx_mode;

typedef enum mgx_info_type { MGX_TYPE_NUMBER = 0, MGX_TYPE_ARRAY = 1, MGX_TYPE_MULTIPLE_ARRAYS = 2 } mgx_info_type;

typedef struct mgx_plan_desc {
  uint32_t struct_size;      /* = sizeof(mgx_plan_desc) */
  uint32_t buffer_size;      /* N: power of two; the GPU path supports 256 <= N <= 4096 */
  double sample_rate;        /* audioContext.sampleRate */
  uint32_t window;           /* mgx_window (Meyda.windowingFunction) */
  uint32_t precision;        /* mgx_precision */
  uint32_t mode;             /* mgx_mode */
  uint32_t num_bark_bands;   /* 24 (loudness.js NUM_BARK_BANDS) */
  uint32_t num_mel_bands;    /* 26 in the reference (mfcc.js:15); 1..64 supported */
  uint32_t num_mfcc_coeffs;  /* 13 (mfcc.js:71) */
  uint32_t scalar_f64;       /* 0: scalar outputs are float32 arrays, 1: float64 */
  int32_t device;            /* HIP device ordinal */
  uint32_t flags;            /* MGX_FLAG_* */
} mgx_plan_desc;

/* mgx_plan_desc.flags */
#define MGX_FLAG_DCT_SEQUENTIAL 1u  /* mfcc.js:85-93 DCT as VALU FMAs in the reference's sequential
                                        order instead of the FP64 matrix cores (the default: same
                                        exact products, f64 sums in 4-band blocks) */
#define MGX_FLAG_MFCC_REFERENCE 2u  /* mfcc.js:53-93 in the reference's own order: each mel band summed
                                        over its bins in ascending order into a float32 accumulator of
                                        double products, Math.log in double, the sequential DCT (MFCC
                                        bit-identical wherever the power spectrum is; slower, see
                                        DESIGN.md §5.3). Default off: segmented-scan mel sums, float32
                                        hardware log, the matrix-core DCT, all within 1e-5. Up to
                                        buffer_size 2048: at 4096 mgx_plan_create refuses the flag
                                        (MGX_E_UNSUPPORTED), whatever the plan's precision and mode. */
#define MGX_FLAG_RESIDENT 4u        /* the real-time path (src/meyda.js:69-91, one buffer per call): one-frame
                                        mgx_extract_host calls are served by one workgroup that stays on the
                                        device between calls, polling a mailbox in pinned host memory, instead
                                        of one launch per call. It holds one CU slot and reads the
                                        mailbox over PCIe (about N x 16 bytes per microsecond; with
                                        MGX_RESIDENT_POLL=light its first word only, ~1 us more per call)
                                        while it waits,
                                        and ends itself 20 ms after its last call (MGX_RESIDENT_IDLE_MS), on
                                        the plan's next call of any other kind, or at mgx_plan_destroy. A device
                                        synchronisation made meanwhile waits for that end. mgx_plan_create
                                        pays the path's one-time set-up (~13 ms: pinned buffers, a hardware
                                        queue, one warm-up call), not the first real-time call. Faithful per-buffer
                                        plans without MGX_FLAG_MFCC_REFERENCE only, up to buffer_size 2048
                                        (MGX_E_UNSUPPORTED otherwise: at 4096 the flag is refused). */

typedef struct mgx_plan mgx_plan;

/* Output arrays, structure of arrays over frames. Any pointer may be NULL: the
 * corresponding feature is then not written (and, where possible, not computed).
 * scalars[i] points to num_frames floats (or doubles if scalar_f64). */
typedef struct mgx_outputs {
  void* scalars[MGX_NUM_SCALARS];
  float* loudness_specific;   /* num_frames x num_bark_bands */
  float* mfcc;                /* num_frames x num_mfcc_coeffs */
  float* amplitude_spectrum;  /* num_frames x N/2 */
  float* power_spectrum;      /* num_frames x N/2 */
  float* complex_real;        /* num_frames x N */
  float* complex_imag;        /* num_frames x N */
} mgx_outputs;

/* Outputs added after mgx_outputs, whose layout is fixed (it carries no size): the mgx_extract_*_ex calls
 * take this struct beside it. It is size-checked, so it can grow: a later field is appended, and a caller
 * built against an older header keeps passing the size it knows. Pointers follow the rules of mgx_outputs
 * (device pointers for the device call, host pointers for the host calls; NULL: not written). */
typedef struct mgx_aux_outputs {
  uint32_t struct_size;   /* = sizeof(mgx_aux_outputs); anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t reserved;      /* 0 */
  float* mel_bands;       /* num_frames x num_mel_bands: loggedMelBands of mfcc.js:53-65, i.e. the
                             Float32Array the reference's DCT reads; row f at mel_bands + f * num_mel_bands */
} mgx_aux_outputs;

/* Host-side tables of a plan (no device needed): used by tests and by bindings
 * that want to show the same tables Meyda exposes (hanning, hamming, barkScale). */
typedef struct mgx_host_tables {
  float* window;        /* N */
  float* hanning;       /* N */
  float* hamming;       /* N */
  float* bark_scale;    /* N */
  int32_t* bark_limits; /* num_bark_bands + 1 */
  int32_t* mel_bins;    /* num_mel_bands + 2 */
  float* dct;           /* num_mfcc_coeffs * num_mel_bands, layout dct[c + j*num_mfcc_coeffs] */
} mgx_host_tables;

void mgx_plan_desc_init(mgx_plan_desc* desc);
int mgx_plan_create(const mgx_plan_desc* desc, mgx_plan** out_plan);
int mgx_plan_destroy(mgx_plan* plan);
int mgx_plan_get_desc(const mgx_plan* plan, mgx_plan_desc* out_desc);

/* Device-resident batch: frames and every non-NULL output are device pointers.
 * Asynchronous on `stream` (hipStream_t or NULL). The launch uses per-stream device scratch,
 * one set per distinct stream the plan launches on: the scalar features' windows (5 KB per
 * resident wave, ~20 MB), for a plan with MGX_FLAG_MFCC_REFERENCE the power-row ring of its mel
 * chains (~2 KB x 8 per resident wave, tens of MB), and at N >= 2048 the tail pool's ticket
 * counter (8 bytes). The whole set is allocated by the first call on its stream, whatever that
 * call's size or outputs (hipMalloc, which may synchronise the device: make one untimed call per
 * stream first, outside any stream capture), and kept until mgx_plan_destroy, which waits for
 * the launches that used it. After that first call a launch keeps no host-side state between
 * calls: it may be captured into a HIP graph and replayed any number of times. */
int mgx_extract_device(mgx_plan* plan, const float* frames, uint64_t num_frames,
                       const mgx_outputs* outputs, void* stream);

/* Host batch: frames and outputs in host memory; returns when the outputs are
 * written. Up to 512 frames run one launch over plan-owned pinned host memory
 * (a single frame of N <= 1024 samples inside the kernel arguments, or with
 * MGX_FLAG_RESIDENT handed to the plan's resident workgroup); larger
 * batches stage through plan-owned device buffers in chunks: two slots of 65,536
 * frames up to N = 2048, and of the same bytes (512 MiB each) above it, 32,768
 * frames at N = 4096. (The pinned buffers of the one-launch path grow with N and the
 * outputs asked for: 512 frames at N = 4096 with every spectrum are 8 MiB of samples
 * and 24 MiB of outputs.) A one-frame call
 * without spectrum outputs may return while the tail of its launch still runs
 * on the plan's stream: later calls on the plan are ordered after it, and
 * mgx_plan_destroy waits for it. */
int mgx_extract_host(mgx_plan* plan, const float* frames, uint64_t num_frames,
                     const mgx_outputs* outputs);

/* Synthetic PCM written straight into HBM:
 * x[i] = (splitmix64(seed + (i+1)*0x9E3779B97F4A7C15) >> 40) * 2^-23 - 1,
 * i = first_frame*N + t for t < num_frames*N. */
int mgx_synth_frames_device(float* frames, uint64_t num_frames, uint32_t buffer_size,
                            uint64_t seed, uint64_t first_frame, void* stream);

int mgx_get_host_tables(const mgx_plan_desc* desc, const mgx_host_tables* out);

/* ---- PCM / WAV ingest ---------------------------------
 * Replaces the browser's decodeAudioData + getChannelData(0) that feed the
 * reference (lib/bufferLoader.js:23, index.html:182, src/meyda.js:72): samples of
 * one channel become float32 exactly as decodeAudioData scales them
 * (u8: (v-128)/128, s16: v/32768, s24: v/2^23, s32: v/2^31, f32: as stored), and
 * are cut into non-overlapping buffer_size frames (a trailing partial frame is
 * dropped, as a ScriptProcessor only delivers full buffers). */
typedef enum mgx_pcm_format {
  MGX_PCM_F32 = 0,
  MGX_PCM_S16 = 1,
  MGX_PCM_U8 = 2,
  MGX_PCM_S24 = 3,   /* packed, 3 bytes little-endian */
  MGX_PCM_S32 = 4
} mgx_pcm_format;

typedef struct mgx_wav_info {
  uint32_t struct_size;     /* = sizeof(mgx_wav_info) */
  uint32_t pcm_format;      /* mgx_pcm_format */
  uint32_t channels;
  uint32_t sample_rate;
  uint32_t bits_per_sample;
  uint32_t block_align;     /* bytes per sample frame (all channels) */
  uint64_t data_offset;     /* byte offset of the first sample in the file */
  uint64_t data_bytes;      /* sample bytes present (the data chunk, clipped to the file) */
  uint64_t sample_frames;   /* data_bytes / block_align */
} mgx_wav_info;

/* RIFF/WAVE header walk: 'fmt ' chunk of 16, 18 or 40 (WAVE_FORMAT_EXTENSIBLE)
 * bytes, PCM (1) or IEEE float (3), chunks in any order, odd sizes padded. Host
 * only (no device). info->struct_size must be set by the caller. */
int mgx_wav_parse(const void* bytes, uint64_t num_bytes, mgx_wav_info* info);

/* Device decode: `sample_frames` interleaved frames of `channels` samples at
 * `pcm` (device memory, any byte alignment) -> float32 samples of channel `channel` at `out`. */
int mgx_pcm_decode_device(const void* pcm, uint64_t sample_frames, uint32_t format, uint32_t channels,
                          uint32_t channel, float* out, void* stream);

/* Host PCM in, host outputs: floor(sample_frames / buffer_size) buffers of channel
 * `channel`. The raw PCM (not float32) crosses PCIe and is decoded on the device;
 * outputs are laid out as for mgx_extract_host. `pcm_bytes` is the size of the buffer at
 * `pcm`: sample_frames * channels * bytes-per-sample beyond it is MGX_E_INVALID_ARGUMENT
 * (no read past the caller's buffer). `pcm` needs no alignment. */
int mgx_extract_host_pcm(mgx_plan* plan, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames,
                         uint32_t format, uint32_t channels, uint32_t channel, const mgx_outputs* outputs);

/* ---- Overlapping buffers of one contiguous signal (hop size) ----------------------
 * Replaces, in a host application, the loop that slices a decoded signal into buffers
 * `hop` samples apart and hands each to the reference (what later Meyda releases call
 * hopSize; the snapshot's ScriptProcessor, src/meyda.js:69-91, only delivers disjoint
 * buffers, hop = buffer_size). The buffers are never materialised: the kernel reads
 * buffer f at samples + f * hop, so the signal is the whole input footprint.
 *
 * A signal of S samples gives F = (S < N) ? 0 : (S - N) / hop + 1 buffers, buffer f being
 * samples [f * hop, f * hop + N); a trailing partial buffer is dropped, as everywhere in
 * this ABI. hop = 0 is MGX_E_INVALID_ARGUMENT; hop > N (samples skipped) is legal; F = 0
 * returns MGX_OK and writes nothing. Outputs are laid out exactly as for
 * mgx_extract_device / mgx_extract_host with num_frames = F, and every output equals, bit
 * for bit, what mgx_extract_device gives on the same F buffers stored densely. The
 * kernel's loads past the last buffer are clamped to buffer F - 1 (its samples
 * [(F - 1) * hop, (F - 1) * hop + N)): nothing beyond that buffer is read, so none of the
 * up to hop - 1 samples of the dropped tail are. Multi-device groups (mgx_group_*) take
 * dense buffers only, and no auxiliary outputs (mgx_aux_outputs, below). */

/* F of the formula above. Host only (no device). */
int mgx_signal_frames(uint64_t num_samples, uint32_t buffer_size, uint32_t hop, uint64_t* num_frames);

/* mgx_extract_device over a device-resident signal: asynchronous on `stream`, with the same
 * per-stream scratch, first-call rule and graph-capture property. `samples` needs only float
 * (4-byte) alignment. */
int mgx_extract_signal_device(mgx_plan* plan, const float* samples, uint64_t num_samples, uint32_t hop,
                              const mgx_outputs* outputs, void* stream);

/* mgx_extract_host over a host signal; F = 1 behaves as mgx_extract_host on the first N
 * samples. Each sample crosses PCIe once per chunk it belongs to, not once per buffer: a
 * chunk of K buffers copies its span of (K - 1) * hop + N samples into the staging slot of
 * the dense path and is extracted there at stride hop, so neighbouring chunks re-send only
 * the N - hop samples they share. The slots stay the dense path's (65,536 * N floats up to
 * N = 2048, 32,768 * N at 4096: a chunk holds at most that many buffers at any hop): for
 * hop > N a chunk holds as many buffers as its span allows there (fewer, down to one for a
 * hop beyond the slot), and a batch small enough for the one-launch path (512 buffers)
 * gathers its buffers densely into the pinned input buffer instead. */
int mgx_extract_signal_host(mgx_plan* plan, const float* samples, uint64_t num_samples, uint32_t hop,
                            const mgx_outputs* outputs);

/* mgx_extract_host_pcm at a hop: decodeAudioData + getChannelData(channel) + the slicing
 * loop. Each chunk's span of raw PCM crosses PCIe and is decoded once on the device. The
 * `pcm_bytes` rule of mgx_extract_host_pcm holds: a short buffer is refused before any copy. */
int mgx_extract_signal_host_pcm(mgx_plan* plan, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames,
                                uint32_t format, uint32_t channels, uint32_t channel, uint32_t hop,
                                const mgx_outputs* outputs);

/* ---- The signal calls with auxiliary outputs -------------------------------------------
 * mgx_extract_signal_device / _host / _host_pcm with a mgx_aux_outputs beside the mgx_outputs. aux = NULL
 * is exactly the corresponding mgx_extract_signal_* call (the six calls above are these with aux = NULL:
 * a dense batch of F buffers is num_samples = F * N, hop = N); with aux, every field of `outputs` may be
 * NULL. The same per-stream scratch, first-call rule, graph-capture property, clamped last loads and
 * pcm_bytes rule hold.
 *
 * aux->mel_bands (feature MGX_MEL_BANDS, "melBands"): for every plan that can compute mfcc -- either
 * precision, literal mode, both windows, 1..64 bands, every flag -- the values the plan's MFCC is the DCT
 * of: with MGX_FLAG_MFCC_REFERENCE the reference-order sums and the double Math.log (the reference's bits
 * wherever the power spectrum is), otherwise the segmented-scan sums and the float32 log (within 1e-5).
 * Asking for it without mfcc runs the mel sums and the log and skips the DCT; asking for it changes no
 * other output in any bit. Rows are num_mel_bands floats apart (4-byte aligned only when that is odd).
 * A silent buffer gives -Infinity in every band, as Math.log(0) does.
 * MGX_FLAG_RESIDENT plans: a one-buffer host call that asks for mel_bands is served by a one-frame launch
 * (the path of a plan without the flag), which first ends the resident workgroup as any other launch
 * does; calls without it go back to the resident workgroup.
 * Multi-device groups (mgx_group_*) take no auxiliary outputs: mgx_packed_layout and MGX_OUT_* are as
 * they were. */
int mgx_extract_device_ex(mgx_plan* plan, const float* samples, uint64_t num_samples, uint32_t hop,
                          const mgx_outputs* outputs, const mgx_aux_outputs* aux, void* stream);
int mgx_extract_host_ex(mgx_plan* plan, const float* samples, uint64_t num_samples, uint32_t hop,
                        const mgx_outputs* outputs, const mgx_aux_outputs* aux);
int mgx_extract_host_pcm_ex(mgx_plan* plan, const void* pcm, uint64_t pcm_bytes, uint64_t sample_frames,
                            uint32_t format, uint32_t channels, uint32_t channel, uint32_t hop,
                            const mgx_outputs* outputs, const mgx_aux_outputs* aux);

/* ---- Buffers at given sample offsets: many signals in one launch ------------------------
 * Replaces, in a host application, the loop over a corpus that slices every clip into buffers and hands
 * each to the reference (src/meyda.js:69-91, one buffer per call; the signal calls above, one clip per
 * call): buffer f of the launch is samples [starts[f], starts[f] + N) of one array, wherever the caller
 * says. One launch then covers every buffer of every clip (mgx_signals_frame_starts), random crops,
 * onset-aligned buffers, or channels stored one after another.
 *
 * Starts in any order are legal: they may repeat, overlap and be odd; `samples` and every buffer need only
 * float (4-byte) alignment. num_frames = 0 returns MGX_OK and writes nothing; num_frames > 0 with starts =
 * NULL or num_samples < N is MGX_E_INVALID_ARGUMENT. Outputs are laid out exactly as for mgx_extract_device
 * with that num_frames, and every output of every plan kind (both precisions, literal mode, both windows,
 * every flag; mel_bands included) equals, bit for bit, what mgx_extract_device gives on the same buffers
 * stored densely. Multi-device groups (mgx_group_*) take dense buffers only; PCM goes through
 * mgx_pcm_decode_device first. */

/* The starts of every buffer of a corpus stored as one array. Replaces the per-clip slicing loop's
 * bookkeeping (src/meyda.js:69-91 delivers the buffers of one source only). Host only (no device).
 * offsets[0..num_signals], non-decreasing: signal s is samples [offsets[s], offsets[s + 1]). Signal s gives
 * mgx_signal_frames(its length, N, hop) buffers, buffer k at offsets[s] + k * hop: no buffer crosses a
 * signal's end. frame_offsets (num_signals + 1 entries, or NULL): the prefix sums of those counts, so signal
 * s's rows of every output are [frame_offsets[s], frame_offsets[s + 1]). starts (or NULL: count only): the
 * start of every buffer, in signal order; capacity: the entries it holds. *num_frames: the total.
 * MGX_E_INVALID_ARGUMENT (nothing written): hop = 0, decreasing offsets, a non-NULL starts with capacity
 * below the total, NULL offsets or num_frames. */
int mgx_signals_frame_starts(const uint64_t* offsets, uint64_t num_signals, uint32_t buffer_size, uint32_t hop,
                             uint64_t* frame_offsets, uint64_t* starts, uint64_t capacity, uint64_t* num_frames);

/* mgx_extract_device (src/meyda.js:69-91,244-261) over buffers at given starts. samples, starts (num_frames
 * entries) and every output are device pointers; asynchronous on `stream`, with the same per-stream scratch,
 * first-call rule and graph-capture property as mgx_extract_device (the table is read by the launch: keep it
 * unchanged until the launch, or every replay of a graph that holds it, has ended). aux as in the _ex calls
 * (NULL allowed). The host cannot see the table, so the kernel reads buffer f at min(starts[f], num_samples - N):
 * nothing outside samples[0, num_samples) is read whatever the table holds, and a start beyond the last whole
 * buffer gives that buffer's outputs. Nothing of `starts` beyond its num_frames entries is read (the kernel's
 * loads past the last buffer are clamped to buffer num_frames - 1, as everywhere in this ABI). */
int mgx_extract_gather_device(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                              uint64_t num_frames, const mgx_outputs* outputs, const mgx_aux_outputs* aux, void* stream);

/* mgx_extract_host over buffers at given starts: host pointers throughout; returns when the outputs are
 * written. A start above num_samples - N is MGX_E_INVALID_ARGUMENT before any copy (the message names its
 * index). Up to 512 buffers are gathered densely into the pinned input buffer and run the one-launch path
 * of mgx_extract_host (one buffer: the kernel-argument frame, or the resident workgroup of a
 * MGX_FLAG_RESIDENT plan). Larger batches go through the two staging slots of the dense path in chunks: a
 * chunk is the longest run of consecutive buffers of at most 65,536 (32,768 at N = 4096) whose span,
 * max(start) + N - min(start), fits a slot (that many times N floats; one buffer always fits). The span crosses PCIe once per chunk, with the
 * chunk's starts (8 bytes per buffer) beside it. Sorted starts -- what mgx_signals_frame_starts gives -- fill
 * their chunks; starts in arbitrary order are served correctly, but every jump of more than a slot ends a
 * chunk, down to one buffer per chunk. */
int mgx_extract_gather_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                            uint64_t num_frames, const mgx_outputs* outputs, const mgx_aux_outputs* aux);

/* ---- Per-signal summaries: mean, variance, min, max of each output over a clip -------------
 * Replaces, in a host application, the loop that pools the per-buffer results of a clip into a clip
 * descriptor (mean and variance of the MFCCs and the scalars; the mean spectrum is the long-term average
 * spectrum). The reference has no counterpart, as with the groups. Both calls are mgx_extract_gather_device /
 * _host with a pooling step behind them: a segmented reduction over the per-frame records on the device, keyed
 * by frame_offsets (num_signals + 1 entries, as mgx_signals_frame_starts writes them): signal s owns rows
 * [frame_offsets[s], frame_offsets[s + 1]) of every output.
 *
 * The statistics are a fixed list, not features (MGX_NUM_FEATURES and the name table are as they were). */
typedef enum mgx_stat {
  MGX_STAT_MEAN = 0,
  MGX_STAT_VARIANCE = 1,  /* population variance (ddof = 0) */
  MGX_STAT_MIN = 2,
  MGX_STAT_MAX = 3,
  MGX_NUM_STATS = 4
} mgx_stat;

/* The summaries of a call, one array per pooled field: field[(s * MGX_NUM_STATS + k) * w + c] is statistic k of
 * column c of signal s, w being the field's floats per frame (1 for a scalar). Every value is a float64, whatever
 * scalar_f64 says. A NULL pointer: the field is not pooled (and, unless asked for per frame, not computed). The
 * complex spectrum has no summary. Size-checked as mgx_aux_outputs is, so it can grow.
 *
 * The values of a column are taken as float64 (every float32 converts exactly). Mean and variance are float64
 * accumulations within 4 F u max|x| and 16 F u R^2 of the exact ones (F rows, u = 2^-53, R = max - min); the
 * variance is never negative, and exactly 0 for a constant column and for a signal of one buffer; min and max
 * are the column's by value. A column with a NaN gives NaN in all four; one with +-Infinity and no NaN (the
 * melBands of a silent buffer) gives mean, min and max as the sum and the comparisons give them and a NaN
 * variance; a signal without buffers gives NaN in all four. A signal's summary is a function of its rows alone:
 * each signal's rows are cut, from its first row, into blocks of 256; a block is summed in ascending row order
 * as (sum of (x - K), sum of (x - K)^2, min, max), K being the signal's first row, and the blocks are added in
 * ascending order. No atomics, and so the same bits from the device call, the host call, a repeated call, any
 * grid, and wherever the host path's chunks end. */
typedef struct mgx_summary_outputs {
  uint32_t struct_size;  /* = sizeof(mgx_summary_outputs); anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t reserved;     /* 0 */
  double* scalars[MGX_NUM_SCALARS];  /* each num_signals x MGX_NUM_STATS */
  double* loudness_specific;         /* num_signals x MGX_NUM_STATS x num_bark_bands */
  double* mfcc;                      /* ... x num_mfcc_coeffs */
  double* amplitude_spectrum;        /* ... x N/2 */
  double* power_spectrum;            /* ... x N/2 */
  double* mel_bands;                 /* ... x num_mel_bands */
} mgx_summary_outputs;

/* The bytes of `workspace` a mgx_summarize_device call with these arguments needs: the per-frame arrays of the
 * fields that are pooled but not requested per frame (outputs and aux, either may be NULL), the table as the
 * kernels read it, the signals' shifts K and the block partials; a multiple of 256, non-decreasing in num_frames,
 * and 0 when there is nothing to keep (no pooled field, no signal, or no buffer). Host only (no device). */
int mgx_summary_workspace_bytes(const mgx_plan* plan, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                                const mgx_summary_outputs* summary, uint64_t num_frames, uint64_t num_signals,
                                uint64_t* bytes);

/* mgx_extract_gather_device, then the summaries. Every pointer is a device pointer, frame_offsets included;
 * asynchronous on `stream`. outputs and aux may be NULL or hold NULL fields; every per-frame field they name
 * is written exactly as mgx_extract_gather_device writes it, bit for bit. Per-frame fields that are pooled
 * but not named, and the partial results, live in `workspace` (256-byte aligned, workspace_bytes of at least
 * mgx_summary_workspace_bytes, else MGX_E_INVALID_ARGUMENT): the call keeps no host-side state and allocates
 * nothing, so it is capturable into a graph under the first-call rule of mgx_extract_device. The host cannot
 * see the table, so the kernels read it as its running maximum limited to num_frames -- entry s as
 * min(max(frame_offsets[0..s]), num_frames): an offset above num_frames is num_frames, an entry below an
 * earlier one gives an empty signal, no row beyond num_frames is read, and nothing outside the num_signals + 1
 * entries is. Every summary array named is written whole (NaN for a signal without buffers, so for every signal
 * when num_frames is 0). num_signals = 0 is the gather call. */
int mgx_summarize_device(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                         uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                         const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                         const mgx_summary_outputs* summary, void* workspace, uint64_t workspace_bytes, void* stream);

/* mgx_extract_gather_host, then the summaries: host pointers throughout; returns when everything is written.
 * The table is checked before any copy: it must be non-decreasing with its last entry at most num_frames
 * (MGX_E_INVALID_ARGUMENT, the message names the index), as a start whose buffer leaves the samples is. The
 * call goes through the staging slots of the chunked path whatever its size (not the one-launch path or the
 * resident workgroup, which it ends as any launch does); each chunk's records are reduced where they lie on
 * the device, a block that a chunk's end cuts going on in the next chunk from its stored state, so only the
 * summaries cross back, plus the per-frame fields named in outputs and aux. */
int mgx_summarize_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                       uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                       const mgx_outputs* outputs, const mgx_aux_outputs* aux, const mgx_summary_outputs* summary);

/* ---- Deltas: the time derivatives of a clip's rows, per frame and pooled ---------------------
 * Replaces, in a host application, the stencil that turns a clip's per-buffer rows into their regression
 * deltas (MFCC + delta + delta-delta, the per-frame vector of HTK, Kaldi and librosa.feature.delta) and the
 * pooling of those into the clip descriptor. The reference has no counterpart. Deltas, like the statistics,
 * are not features: MGX_NUM_FEATURES, the name table and every struct above are as they were.
 *
 * A signal owns rows [a, b) of an array of num_frames rows x cols columns (row-major, rows cols elements
 * apart). For a half-width W (1 .. MGX_DELTA_MAX_WIDTH), a row t of [a, b) and a column c:
 *
 *   x~(u)     = x(min(max(u, a), b - 1), c)          rows outside the signal repeat its first / last row
 *   delta(t,c) = (sum_{n = 1..W} n (x~(t + n) - x~(t - n))) / D,   D = 2 sum n^2 = W (W + 1) (2 W + 1) / 3
 *
 * The values are taken as float64 (a float32 converts exactly); the sum runs in ascending n in float64 (a
 * difference, a product and an addition per term, each rounded), is divided by D and rounded once to the
 * array's element type. The second order is the same operator over the delta rows as stored, clamped again at
 * the signal's own ends: bit for bit what a second call on the first call's output gives. Non-finite values
 * follow IEEE (Inf - Inf = NaN) and reach the rows within W (2 W for the second order) of them, in their own
 * signal and column. A signal of one row has delta 0 wherever x is finite; an empty signal writes nothing;
 * rows that belong to no signal (before frame_offsets[0], from frame_offsets[num_signals] on) are not written.
 * A value is a function of its own signal's rows alone: no atomics, and the same bits from every call below,
 * from a repeated call and from any grid. */
#define MGX_DELTA_MAX_WIDTH 8

/* The operator on device arrays; no plan (as mgx_pcm_decode_device takes none): asynchronous on `stream`, no
 * allocation, no host-side state, capturable. rows_f64: 0 float32 rows, 1 float64 rows (the scalars of a
 * scalar_f64 plan); the outputs have the rows' element type and shape. delta: the first order, delta2: the
 * second; either may be NULL (with delta2 alone the first order is recomputed where the second needs it, from
 * the same arithmetic: the same bits). frame_offsets: num_signals + 1 entries in device memory, or NULL with
 * num_signals = 0 for one signal [0, num_frames) -- the output of a mgx_extract_signal_* call. The table is
 * read as given, every entry limited to num_frames: a non-decreasing one gives the definition above, any other
 * gives unspecified values in the outputs and no access outside the arrays.
 * MGX_E_INVALID_ARGUMENT before any launch: cols = 0, width outside 1 .. MGX_DELTA_MAX_WIDTH, rows_f64 > 1,
 * both outputs NULL, an output equal to rows or to the other output, num_signals > 0 with NULL frame_offsets,
 * NULL rows with num_frames > 0. num_frames = 0 returns MGX_OK and writes nothing. */
int mgx_delta_device(const void* rows, uint64_t num_frames, uint32_t cols, uint32_t rows_f64,
                     const uint64_t* frame_offsets, uint64_t num_signals, uint32_t width,
                     void* delta, void* delta2, void* stream);

/* The summaries of the delta rows beside the summaries of the rows: mgx_summarize_* with this struct behind
 * their arguments. delta / delta2 are mgx_summary_outputs themselves (same layout, float64 values and four
 * statistics) and name the fields whose first / second order rows are pooled -- by the summary kernels, so
 * every rule of the summaries holds for them (the bounds, NaN for an empty signal, NaN in all four for a
 * column with a NaN, blocks of 256 rows from the signal's first row); a one-buffer signal gives mean = min =
 * max = 0 and variance exactly 0. Fields: the 13 scalars (float64 rows on a scalar_f64 plan), loudness_specific,
 * mfcc and mel_bands; a spectrum is MGX_E_UNSUPPORTED (the operator itself takes any cols). delta2 may name
 * fields delta does not. */
typedef struct mgx_delta_summaries {
  uint32_t struct_size;                  /* = sizeof(mgx_delta_summaries); anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t width;                        /* W */
  const mgx_summary_outputs* delta;      /* summaries of the delta rows of the fields it names, or NULL */
  const mgx_summary_outputs* delta2;     /* of the second-order rows, or NULL */
} mgx_delta_summaries;

/* The three summary calls with deltas. deltas = NULL is exactly the mgx_summarize_* call (and the bytes of
 * mgx_summary_workspace_bytes); `summary` must be a valid struct, but all of its fields may be NULL. Every
 * per-frame field and every base summary the call names is written bit for bit as mgx_summarize_device /
 * _host writes it.
 * Device call: the workspace also holds the rows of a delta'd field that is neither requested per frame nor
 * pooled, the delta and second-order rows of the named fields and their partials; its bytes keep the contract
 * of mgx_summary_workspace_bytes (a multiple of 256, non-decreasing in num_frames, 0 when there is nothing to
 * keep). After the gather launch the operator runs over those rows (two passes per field, keyed by the table
 * as the summary kernels read it), then the summary kernels.
 * Host call: the base summaries are reduced chunk by chunk as in mgx_summarize_host; the rows of the delta'd
 * fields alone are copied, device to device, into plan-owned arrays as long as the call (at most 3 x
 * num_frames x their columns x 4 bytes, 8 for float64 scalars; grown on demand, freed at mgx_plan_destroy;
 * MGX_E_OUT_OF_MEMORY when the device has no room), and after the last chunk the operator and the pooling run
 * over them as in the device call: the device call's bits, wherever the chunks end. Only summaries and the
 * per-frame fields named cross back. */
int mgx_summarize_deltas_workspace_bytes(const mgx_plan* plan, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                                         const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                                         uint64_t num_frames, uint64_t num_signals, uint64_t* bytes);
int mgx_summarize_deltas_device(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                                uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                                const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                                const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                                void* workspace, uint64_t workspace_bytes, void* stream);
int mgx_summarize_deltas_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                              uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                              const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                              const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas);

/* ---- Spectral flux: the change between a clip's rows, per frame and pooled --------------------
 * Replaces, in a host application, the loop that compares every buffer's row (its amplitude spectrum, its
 * log-mel bands, its MFCCs) with an earlier buffer's row of the same clip: the onset-strength envelope of onset
 * and beat detection (Dixon's half-wave rectified flux, the L2 flux of Marsyas, librosa.onset.onset_strength
 * over log-mel rows). The reference delivers one buffer per call and has no counterpart. Flux, like the
 * statistics and the deltas, is not a feature: MGX_NUM_FEATURES, the name table and every struct above are as
 * they were.
 *
 * A signal owns rows [a, b) of an array of num_frames rows x cols columns (row-major). For a lag L
 * (1 .. MGX_FLUX_MAX_LAG), a row t of [a, b) and p = max(t - L, a) -- the earlier row, clamped at the signal's
 * first row as the deltas clamp:
 *
 *   d(c) = +0 if x(t,c) == x(p,c), else x(t,c) - x(p,c)      values taken as float64 (a float32 converts
 *                                                            exactly), the difference rounded once
 *   e(c) = d if d > 0 or d is NaN, else +0    MGX_FLUX_RECTIFIED
 *          |d|                                MGX_FLUX_L1
 *          d d, rounded before it is added    MGX_FLUX_L2
 *
 * The equality rule keeps a column that is -Infinity in both rows (a mel band that spans no bin) at 0 instead
 * of Inf - Inf; a NaN compares unequal and stays NaN. The terms are added in a fixed order: 64 partials P[l]
 * start at +0; for k = 0, 64, 128, ... ascending, P[l] += e(k + l) for the columns that exist; then P[l] +=
 * P[l + h] for l < h, with h = 32, 16, 8, 4, 2, 1; S = P[0]. Every term is >= +0 or NaN, so a partial that
 * stayed +0 changes nothing, and no mapping of rows to lanes changes a bit. The result is S (RECTIFIED, L1) or
 * sqrt(S) in float64 as the device's sqrt gives it (L2), rounded once to the rows' element type. A signal's first row,
 * and every row of a one-row signal, is 0 wherever the row is finite; an empty signal writes nothing; rows that
 * belong to no signal are not written. A value is a function of its own signal's rows alone: no atomics, and
 * the same bits from every call below, from a repeated call and from any grid. */
typedef enum mgx_flux_mode {
  MGX_FLUX_RECTIFIED = 0,
  MGX_FLUX_L1 = 1,
  MGX_FLUX_L2 = 2,
  MGX_NUM_FLUX_MODES = 3
} mgx_flux_mode;
#define MGX_FLUX_MAX_LAG 8

/* The operator on device arrays; no plan: asynchronous on `stream`, no allocation, no host-side state,
 * capturable. rows_f64: 0 float32 rows, 1 float64 rows; flux: num_frames values of the rows' element type.
 * frame_offsets: num_signals + 1 entries in device memory, or NULL with num_signals = 0 for one signal
 * [0, num_frames). The table is read as mgx_delta_device reads it, every entry limited to num_frames: a
 * non-decreasing one gives the definition above, any other gives unspecified values and no access outside the
 * arrays.
 * MGX_E_INVALID_ARGUMENT before any launch: cols = 0, mode >= MGX_NUM_FLUX_MODES, lag outside 1 ..
 * MGX_FLUX_MAX_LAG, rows_f64 > 1, NULL flux, flux equal to rows, num_signals > 0 with NULL frame_offsets, NULL
 * rows with num_frames > 0. num_frames = 0 returns MGX_OK and writes nothing. */
int mgx_flux_device(const void* rows, uint64_t num_frames, uint32_t cols, uint32_t rows_f64,
                    const uint64_t* frame_offsets, uint64_t num_signals, uint32_t mode, uint32_t lag,
                    void* flux, void* stream);

/* One flux of one field through the summary calls: its column per frame, its pooling per clip, or both. */
typedef struct mgx_flux_request {
  uint32_t struct_size;  /* = sizeof(mgx_flux_request), 32; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t field;        /* MGX_LOUDNESS (the loudness_specific rows), MGX_MFCC, MGX_AMPLITUDE_SPECTRUM,
                            MGX_POWER_SPECTRUM or MGX_MEL_BANDS; anything else: MGX_E_UNSUPPORTED */
  uint32_t mode, lag;
  float* per_frame;      /* num_frames floats (the onset envelope), or NULL */
  double* summary;       /* num_signals x MGX_NUM_STATS: mean, variance, min, max of the flux per clip, or NULL */
} mgx_flux_request;
#define MGX_FLUX_MAX_REQUESTS 4

/* The three mgx_summarize_deltas_* calls with num_flux requests behind `deltas` (which may be NULL). num_flux =
 * 0 is exactly the deltas call, its workspace bytes included. MGX_E_INVALID_ARGUMENT: more than
 * MGX_FLUX_MAX_REQUESTS requests, a bad struct_size, mode or lag, a request with both pointers NULL, summary set
 * with num_signals = 0. Everything the deltas call writes is written bit for bit as before. num_signals = 0 is
 * the gather call, as in every summary call: no signal owns a row, and no per_frame column is written.
 * Device call: the workspace also holds the rows of a flux'd field that nothing else keeps (a field requested
 * per frame, pooled or delta'd is shared), the flux column of a request without per_frame, and the pooling's
 * shifts and partials; its bytes keep the contract of mgx_summary_workspace_bytes. After the gather launch the
 * operator runs per request, keyed by the table as the summary kernels read it, then the summary kernels over
 * the one-column flux array: every rule of the summaries holds for it.
 * Host call: the device call's bits wherever the chunks end. No spectrum is kept for the call: the last lag
 * rows of each flux'd field go from a chunk to a small plan-owned carry buffer before the slot is reused, the
 * operator runs per chunk over the slot's rows and that carry, and the flux columns alone (4 bytes per buffer
 * and request; grown on demand, freed at mgx_plan_destroy) last as long as the call and are pooled after the
 * last chunk. Only summaries, per_frame columns and the per-frame fields named cross back; of a per_frame column
 * the rows of the signals alone, [frame_offsets[0], frame_offsets[num_signals]): a row that belongs to no signal
 * is not written, as in the device call. */
int mgx_summarize_flux_workspace_bytes(const mgx_plan* plan, const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                                       const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                                       const mgx_flux_request* flux, uint32_t num_flux, uint64_t num_frames,
                                       uint64_t num_signals, uint64_t* bytes);
int mgx_summarize_flux_device(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                              uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                              const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                              const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                              const mgx_flux_request* flux, uint32_t num_flux,
                              void* workspace, uint64_t workspace_bytes, void* stream);
int mgx_summarize_flux_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                            uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                            const mgx_outputs* outputs, const mgx_aux_outputs* aux,
                            const mgx_summary_outputs* summary, const mgx_delta_summaries* deltas,
                            const mgx_flux_request* flux, uint32_t num_flux);

/* ---- Onsets: the peaks of a clip's envelope, picked on the device ------------------------------
 * Replaces, in a host application, the loop that runs over the flux column after it was copied back: a moving
 * maximum, a moving mean, a threshold and a greedy minimum distance (librosa.util.peak_pick, with the edges
 * handled as this library handles them). With it, envelope -> onsets -> onset-aligned starts -> a second gather
 * launch runs without a host round trip. The reference has no counterpart. Like the statistics, the deltas and
 * the flux it is no feature: MGX_NUM_FEATURES, the name table and every struct above are as they were.
 *
 * A signal owns rows [a, b) of a one-column envelope x of num_frames values, float32 or float64; values are
 * taken as float64. Rows outside the signal repeat its first or last row, as for the deltas:
 * x~(u) = x(min(max(u, a), b - 1)). The parameters are pre_max, post_max, pre_avg, post_avg (each 0 ..
 * MGX_PEAK_MAX_REACH), delta (a double, not NaN) and wait (any uint32). Row t of [a, b) is a candidate if
 *
 *   1. no u in [t - pre_max, t + post_max] has x~(u) > x(t) -- an IEEE comparison: a NaN neighbour does not
 *      block --, and
 *   2. x(t) >= m + delta, where m starts at +0, m += x~(u) for u = t - pre_avg .. t + post_avg ascending, each
 *      addition rounded to float64; m is then divided by (pre_avg + post_avg + 1) and rounded once, delta is
 *      added and the sum rounded once. A NaN on either side makes the comparison false: a NaN row is never a
 *      candidate, and a NaN inside the averaging window rejects the row.
 *
 * The peaks of the signal are chosen from its candidates in ascending order: the first candidate is a peak; a
 * later candidate t is a peak iff t - (the last peak) > wait. A peak is a function of its own signal's rows
 * alone; rows of no signal are never peaks and are never written; an empty signal has no peaks. No atomics:
 * every call below, a repeated call and any grid give the same values (integers all, so the same bits). */
#define MGX_PEAK_MAX_REACH 64
typedef struct mgx_peak_params {
  uint32_t struct_size;  /* = sizeof(mgx_peak_params), 32; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t pre_max, post_max, pre_avg, post_avg, wait;
  double delta;
} mgx_peak_params;
typedef struct mgx_peak_outputs {
  uint32_t struct_size;    /* = sizeof(mgx_peak_outputs), 56 */
  uint32_t reserved;
  uint8_t* mask;           /* num_frames, 1 = peak, 0 = row of a signal that is no peak; or NULL */
  uint64_t* peak_offsets;  /* S + 1 entries: signal s's peaks are peaks[peak_offsets[s] .. peak_offsets[s+1]); or NULL */
  uint64_t* peaks;         /* row indices of the whole array, ascending; `capacity` entries; or NULL */
  uint64_t capacity;
  const uint64_t* starts;  /* optional: the gather table the rows came from ...                       */
  uint64_t* peak_starts;   /* ... and starts[peaks[i]] for every peak written: the next launch's table */
} mgx_peak_outputs;

/* The bytes mgx_peaks_device works in: a multiple of 256, non-decreasing in both arguments (bitmaps of one bit
 * per row and the scan's block sums: about half a byte per row). Host only. */
int mgx_peaks_workspace_bytes(uint64_t num_frames, uint64_t num_signals, uint64_t* bytes);

/* The picker on device arrays; no plan: asynchronous on `stream`, no allocation, no host-side state, capturable.
 * Every pointer is a device pointer. envelope_f64: 0 float32, 1 float64. S is num_signals, or 1 when
 * frame_offsets is NULL and num_signals is 0: one signal [0, num_frames). The table is read as mgx_delta_device
 * reads it, every entry limited to num_frames: a non-decreasing one gives the definition above, any other gives
 * unspecified values, and no access is made outside the arrays -- no write to peaks or peak_starts at or beyond
 * `capacity` either. peak_offsets always holds the true counts; of peaks (and peak_starts) the first
 * min(total, capacity) entries are written, so a caller can size the list and call again. num_frames = 0 writes
 * peak_offsets (all 0) and nothing else.
 * MGX_E_INVALID_ARGUMENT before any launch: a bad struct_size in either struct, a reach above
 * MGX_PEAK_MAX_REACH, a NaN delta, envelope_f64 > 1, mask, peak_offsets and peaks all NULL, peaks set with
 * capacity 0, peak_starts without starts or without peaks, num_signals > 0 with NULL frame_offsets, NULL envelope
 * with num_frames > 0, a workspace smaller than mgx_peaks_workspace_bytes or not 256-byte aligned. */
int mgx_peaks_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64,
                     const uint64_t* frame_offsets, uint64_t num_signals, const mgx_peak_params* params,
                     const mgx_peak_outputs* out, void* workspace, uint64_t workspace_bytes, void* stream);

/* Host pointers throughout: mgx_summarize_flux_host with exactly the one request `flux` (no other output, summary
 * or delta), followed by the picker. flux->per_frame and flux->summary are honoured when set and written bit for
 * bit as that call writes them; unlike there, both may be NULL. The picker runs once, after the last chunk, over
 * the plan-owned flux column the flux host path keeps on the device for the length of the call: the envelope is
 * not uploaded again, and only peak_offsets, peaks and what the request names cross back. The result equals
 * mgx_peaks_device on the column mgx_summarize_flux_host returns, wherever the chunks end.
 * peak_offsets: num_signals + 1 entries, non-NULL (the true counts); peaks: `capacity` entries, the first
 * min(total, capacity) written, or NULL with capacity 0 for the counts alone. num_signals = 0 is
 * MGX_E_INVALID_ARGUMENT: onsets need signals. Every other refusal is that of the two calls it is made of. */
int mgx_onsets_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                    uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                    const mgx_flux_request* flux, const mgx_peak_params* params,
                    uint64_t* peak_offsets, uint64_t* peaks, uint64_t capacity);

/* ---- Chroma: pitch-class profiles of a clip's spectra, per frame and pooled ------------------------
 * Replaces, in a host application, the product of every buffer's amplitude spectrum with a chroma filter bank
 * after the spectrum was copied back: later Meyda's `chroma` (src/extractors/chroma.js with
 * createChromaFilterBank of src/utilities.js, a port of librosa.filters.chroma). The reference snapshot has no
 * counterpart, so both halves are stated here in full. Chroma, like the statistics, the deltas, the flux and the
 * peaks, is not a feature: MGX_NUM_FEATURES, the name table and every struct above are as they were.
 *
 * The filter bank (mgx_chroma_weights; host only, no device is touched). N = buffer_size, sr = sample_rate,
 * C = num_chroma; everything in float64, rounded once to float32 at the end (positive stays positive, below). For k = 0 .. N/2:
 *
 *   fb(k)  = C log2((k sr / N) / (a440 / 16))  for k >= 1;   fb(0) = fb(1) - 1.5 C
 *   bw(k)  = max(fb(k + 1) - fb(k), 1)         for k < N/2
 *   h      = C / 2 rounded to the nearest integer, ties to even
 *   d(c,k) = ((fb(k) - c + h) mod C) - h       the mod taken in [0, C)
 *   w(c,k) = exp(-0.5 (2 d / bw(k))^2)
 *
 * then (1) every column k is divided by sqrt(sum_c w(c,k)^2); (2) if octave_width > 0 it is multiplied by
 * exp(-0.5 ((fb(k) / C - center_octave) / octave_width)^2); (3) if base_c, row c of the result is row
 * (c + 3 (C div 12)) mod C of the table so far (row 0 is C instead of A). Columns 0 .. N/2 - 1 are kept: the bins
 * the amplitude spectrum has. The one rounding is to the nearest float32, except that a positive value below the
 * smallest float32 (2^-149) becomes that value and not +0: from C = 15 on the far rows of a narrow bin (bw = 1,
 * |d| above 7.2: exp(-2 d^2) down to exp(-648) at C = 36) are that small. So every entry is finite and > 0, as the
 * table is in float64, and under it an overflowed amplitude is +Infinity in every output of its row, not 0 x Inf.
 * MGX_E_INVALID_ARGUMENT: a NULL pointer, a bad struct_size, C outside 1 .. MGX_CHROMA_MAX_BINS, sample_rate, a440
 * or octave_width not finite or not positive (octave_width may be 0: no octave weighting).
 * MGX_E_NOT_POWER_OF_TWO: buffer_size is not a power of two, or is below 4. */
#define MGX_CHROMA_MAX_BINS 36
typedef struct mgx_chroma_params {
  uint32_t struct_size;   /* = sizeof(mgx_chroma_params), 40; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t num_chroma;    /* C, 1 .. MGX_CHROMA_MAX_BINS; 12 */
  double a440;            /* 440 */
  double center_octave;   /* 5 */
  double octave_width;    /* 2; 0: no octave weighting */
  uint32_t base_c;        /* 1: row 0 is C; 0: row 0 is A */
  uint32_t reserved;
} mgx_chroma_params;
void mgx_chroma_params_init(mgx_chroma_params* params);
int mgx_chroma_weights(uint32_t buffer_size, double sample_rate, const mgx_chroma_params* params,
                       float* weights /* C x N/2, row-major */);

/* The operator: chroma(t, c) of a row x(t, .) of `cols` float32 values under a bank w of C x cols float32 values.
 * Values are taken as float64; a product w(c,k) x(k) of two float32 is exact there. Per output c the products are
 * added in a fixed order: 64 partials P[l] start at +0; for k = 0, 64, 128, ... ascending, P[l] += w(c,k+l) x(k+l)
 * for the columns that exist, each addition rounded; then P[l] += P[l + h] for l < h, with h = 32, 16, 8, 4, 2, 1;
 * S(c) = P[0]. MGX_CHROMA_NORM_MAX is Meyda's v / max: m starts at -Infinity; for c ascending, m = S(c) if
 * S(c) > m (an IEEE comparison: a NaN never becomes m); if m > 0 and m is finite, S(c) = S(c) / m, one correctly
 * rounded float64 division per output; otherwise the row is left as it is (a silent buffer, a row whose sums are
 * all <= 0 under a caller's signed bank, an infinite maximum). The result is rounded once to float32. Non-finite
 * inputs follow IEEE: a NaN or an overflowed amplitude reaches the outputs of its own row only. A partial starts
 * at +0, so no sum is -0. The bank is the caller's: it may be signed, and its rows need not be pitch classes
 * (octave bands, a tonnetz projection). Rows are independent: no table of signals, no atomics, and the same bits
 * from every call below, from a repeated call and from any grid. */
typedef enum mgx_chroma_norm {
  MGX_CHROMA_NORM_NONE = 0,
  MGX_CHROMA_NORM_MAX = 1,
  MGX_NUM_CHROMA_NORMS = 2
} mgx_chroma_norm;

/* The operator on device arrays; no plan: asynchronous on `stream`, no allocation, no host-side state,
 * capturable. rows: num_frames x cols float32; weights: C x cols float32; chroma: num_frames x C float32.
 * MGX_E_INVALID_ARGUMENT before any launch: cols = 0, C outside 1 .. MGX_CHROMA_MAX_BINS, norm >=
 * MGX_NUM_CHROMA_NORMS, NULL weights or chroma, chroma equal to rows or to weights, NULL rows with
 * num_frames > 0. num_frames = 0 returns MGX_OK and writes nothing. */
int mgx_chroma_device(const float* rows, uint64_t num_frames, uint32_t cols, const float* weights /* device */,
                      uint32_t num_chroma, uint32_t norm, float* chroma, void* stream);

typedef struct mgx_chroma_request {
  uint32_t struct_size;  /* = sizeof(mgx_chroma_request), 40; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t num_chroma;   /* C */
  uint32_t norm;         /* mgx_chroma_norm */
  uint32_t reserved;
  const float* weights;  /* host, C x N/2 */
  float* per_frame;      /* num_frames x C, or NULL */
  double* summary;       /* num_signals x MGX_NUM_STATS x C: mean, variance, min, max per clip, or NULL */
} mgx_chroma_request;

/* Host pointers throughout: mgx_extract_gather_host with the amplitude spectrum as a field that is laid out in
 * the staging slot and does not cross back. Behind each chunk's extraction the operator runs over the chunk's
 * amplitude rows where they lie and writes its rows of a plan-owned num_frames x C float32 array that lasts as
 * long as the call (grown on demand, freed at mgx_plan_destroy); the weights are uploaded once per call. After the
 * last chunk per_frame is copied back and, if summary is set, the summary kernels pool the array as one field of
 * width C keyed by the table: every rule of the summaries holds (blocks of 256 rows from the signal's first row,
 * NaN in all four for a signal without buffers, no atomics). Only C floats per buffer and the summaries cross
 * back. The result equals mgx_chroma_device on the amplitude rows mgx_extract_gather_host returns, bit for bit,
 * wherever the chunks end. The call goes through the staging slots whatever its size and ends a resident
 * workgroup as any launch does.
 * The table and the starts are checked as mgx_summarize_host checks them, before any copy; frame_offsets may be
 * NULL with num_signals = 0 and per_frame alone. MGX_E_INVALID_ARGUMENT also for: summary with num_signals = 0,
 * both outputs NULL, NULL weights, a bad struct_size, C or norm. */
int mgx_chroma_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                    uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                    const mgx_chroma_request* request);

/* ---- Tempo: a clip's autocorrelation tempogram and tempo on the device ---------------------------
 * Replaces, in a host application, the local autocorrelation of the onset envelope after it was copied back, its
 * average over the clip and the weighing of the lags with a tempo prior (librosa.feature.tempogram and
 * librosa.feature.tempo). The reference snapshot has no counterpart, so the definitions are stated here in full.
 * Like the statistics, the deltas, the flux, the peaks and the chroma it is no feature: MGX_NUM_FEATURES, the name
 * table and every struct above are as they were.
 *
 * The tempogram. A signal owns rows [a, b) of a one-column envelope x of num_frames values, float32 or float64;
 * values are taken as float64. Outside the signal the envelope is +0, not an edge repeat: x~(u) = x(u) for
 * a <= u < b, else +0. The parameters are the window length W (2 .. MGX_TEMPOGRAM_MAX_WIN), the number of lags L
 * (1 .. W), a window h of W float32 values (the caller's, as chroma's bank is) and a normalisation. For row t of
 * [a, b):
 *
 *   1. y(j) = h(j) x~(t - floor(W / 2) + j), j = 0 .. W - 1, formed in float64 and rounded once to float32
 *      (denormal results are kept).
 *   2. For l = 0 .. L - 1: S(l) starts at +0; S(l) += y(j) y(j + l) for j = 0, 1, .., W - 1 - l ascending. The
 *      product of two float32 values is exact in float64; each addition is rounded once (an FMA rounds what the
 *      definition rounds). The order is plainly sequential on purpose: a lane can own a lag.
 *   3. MGX_TEMPOGRAM_NORM_NONE leaves S as it is.
 *   4. MGX_TEMPOGRAM_NORM_LAG0: if S(0) > 0 and S(0) is finite, S(l) = S(l) / S(0), one correctly rounded float64
 *      division per output (lag 0 becomes exactly 1); otherwise the row is left as it is (a silent window, a NaN,
 *      an overflow).
 *   5. The result is rounded once to float32.
 *
 * Non-finite inputs follow IEEE: a NaN or an infinite envelope value reaches the rows whose window holds it, in
 * its own signal, and no other row. Rows that belong to no signal are not written; an empty signal has no rows.
 * No atomics: the same bits from every call below, a repeated call, a graph replay and any grid.
 *
 * The window (mgx_tempogram_window; host only): the periodic Hann window h(j) = 0.5 - 0.5 cos(2 pi j / W), formed
 * in float64 and rounded once to float32. MGX_E_INVALID_ARGUMENT: W outside 2 .. MGX_TEMPOGRAM_MAX_WIN, NULL h.
 *
 * The prior (mgx_tempo_prior; host only): p(0) = 0; for l >= 1 with bpm(l) = 60 frame_rate / l: p(l) = 0 if
 * max_bpm > 0 and bpm(l) > max_bpm, otherwise p(l) = exp(-0.5 ((log2 bpm(l) - log2 start_bpm) / std_octaves)^2):
 * librosa's log-normal prior without its constant factor (its defaults: 120, 1.0, 320). All float64.
 * MGX_E_INVALID_ARGUMENT: frame_rate, start_bpm or std_octaves not finite or not positive, max_bpm NaN or
 * negative, L = 0, NULL p.
 *
 * The pick takes a mean row m(.) of L doubles, the weights p and a gain g (1e6 in librosa; finite and >= 0):
 * s(l) = (1 + g m(l)) p(l), three float64 roundings and no contraction. The lag is the lowest l whose s(l) is
 * greater than every s before it, starting from a best of +0: a NaN never wins, and no positive score gives lag
 * 0, "none". This is the argmax of librosa's log1p(g m) + log p with the monotone exponential applied, so the
 * device evaluates no transcendental. The output is a uint32 per signal; bpm = 60 frame_rate / lag is the
 * binding's arithmetic. */
#define MGX_TEMPOGRAM_MAX_WIN 1024
typedef enum mgx_tempogram_norm {
  MGX_TEMPOGRAM_NORM_NONE = 0,
  MGX_TEMPOGRAM_NORM_LAG0 = 1,
  MGX_NUM_TEMPOGRAM_NORMS = 2
} mgx_tempogram_norm;
typedef struct mgx_tempo_params {
  uint32_t struct_size;  /* = sizeof(mgx_tempo_params), 24; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t win_length;   /* W, 2 .. MGX_TEMPOGRAM_MAX_WIN; 384 */
  uint32_t num_lags;     /* L, 1 .. W; 384 */
  uint32_t norm;         /* mgx_tempogram_norm; MGX_TEMPOGRAM_NORM_LAG0 */
  double gain;           /* g of the pick, finite and >= 0; 1e6 */
} mgx_tempo_params;
void mgx_tempo_params_init(mgx_tempo_params* params);
int mgx_tempogram_window(uint32_t win_length, float* window /* W */);
int mgx_tempo_prior(double frame_rate, double start_bpm, double std_octaves, double max_bpm, uint32_t num_lags,
                    double* prior /* L */);

/* The tempogram on device arrays; no plan: asynchronous on `stream`, no allocation, no host-side state, capturable.
 * Every pointer is a device pointer. envelope_f64: 0 float32, 1 float64. frame_offsets NULL with num_signals 0:
 * one signal [0, num_frames). The table is read as mgx_delta_device reads it, every entry limited to num_frames:
 * a non-decreasing one gives the definition above, any other gives unspecified values in the rows it is wrong
 * about, and no access is made outside the arrays. tempogram: num_frames x L float32. num_frames = 0 returns
 * MGX_OK and writes nothing.
 * MGX_E_INVALID_ARGUMENT before any launch: envelope_f64 > 1, W outside 2 .. MGX_TEMPOGRAM_MAX_WIN, L outside
 * 1 .. W, norm >= MGX_NUM_TEMPOGRAM_NORMS, NULL window or tempogram, tempogram equal to envelope or to window,
 * num_signals > 0 with NULL frame_offsets, NULL envelope with num_frames > 0. */
int mgx_tempogram_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64,
                         const uint64_t* frame_offsets, uint64_t num_signals, const float* window /* device */,
                         uint32_t win_length, uint32_t num_lags, uint32_t norm, float* tempogram, void* stream);

/* Tempogram -> per-clip pooling -> pick, on device arrays; no plan, no allocation, capturable. Outputs, each
 * optional but not all NULL: tempogram (num_frames x L float32), summary (S x MGX_NUM_STATS x L doubles: the
 * tempogram rows pooled per clip by the summary kernels as one field of width L, every rule of the summaries
 * holding: blocks of 256 rows from the signal's first row, NaN in all four for an empty signal), lag (S uint32:
 * the pick over the mean row under `prior`, L doubles on the device, required with lag). S is num_signals, or 1
 * when frame_offsets is NULL and num_signals is 0. The table is made non-decreasing and limited to num_frames as
 * mgx_summarize_device makes it.
 * With a tempogram output the rows are written there and pooled in one pass. Without one they are produced
 * MGX_TEMPO_CHUNK_ROWS rows at a time into the workspace and each pass is pooled by a partial launch over its
 * rows, so the workspace does not grow with num_frames x L; both routes give the same bits.
 * mgx_tempo_workspace_bytes (host only; keep_rows: 1 when the call has a tempogram output): a multiple of 256,
 *   256 ceil((S + 1) 8 / 256) + 256 ceil(S L 8 / 256) + 256 ceil((floor(F / 256) + S + 1) 5 L 8 / 256)
 *   + 256 ceil(S 4 L 8 / 256) + (keep_rows ? 0 : 256 ceil(min(F, MGX_TEMPO_CHUNK_ROWS) L 4 / 256))
 * -- the table, the shifts, the partials, the summaries and a pass of rows (100,663,296 bytes at L = 384).
 * MGX_E_INVALID_ARGUMENT before any launch: what mgx_tempogram_device refuses, a bad struct_size, a gain that is
 * not finite or is negative, all three outputs NULL, lag without prior, a workspace smaller than
 * mgx_tempo_workspace_bytes or not 256-byte aligned. */
#define MGX_TEMPO_CHUNK_ROWS 65536
int mgx_tempo_workspace_bytes(uint64_t num_frames, uint64_t num_signals, const mgx_tempo_params* params,
                              uint32_t keep_rows, uint64_t* bytes);
int mgx_tempo_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                     uint64_t num_signals, const mgx_tempo_params* params, const float* window /* device */,
                     const double* prior /* device */, float* tempogram, double* summary, uint32_t* lag,
                     void* workspace, uint64_t workspace_bytes, void* stream);

/* Host pointers throughout: mgx_summarize_flux_host with exactly the one request `flux` (no other output, summary
 * or delta), followed by mgx_tempo_device without a tempogram output over the plan-owned flux column that call
 * keeps on the device -- as mgx_onsets_host runs the picker. flux->per_frame and flux->summary are honoured when
 * set and written bit for bit as that call writes them; both may be NULL. window (W floats) and prior (L doubles,
 * required with lag) are uploaded once per call. Only lag (S uint32), summary (S x MGX_NUM_STATS x L doubles) and
 * what the request names cross back; summary or lag may be NULL, not both. The result equals mgx_tempo_device on
 * the column mgx_summarize_flux_host returns, wherever the chunks end. num_signals = 0 is
 * MGX_E_INVALID_ARGUMENT: a tempo is a clip's. Every other refusal is that of the two calls it is made of. */
int mgx_tempo_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                   uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                   const mgx_flux_request* flux, const mgx_tempo_params* params, const float* window,
                   const double* prior, double* summary, uint32_t* lag);

/* ---- Beats: a clip's beats by dynamic programming on the device ------------------------------------
 * Replaces, in a host application, the loop that places the beats on the onset envelope after it was copied back
 * (librosa.beat.beat_track's tracker: a local score, a cumulative score with a log-squared penalty on the distance
 * to the beat before, the last beat at a late local maximum, the chain of back links, a trim of weak ends). With it,
 * envelope -> tempo -> beats -> beat-aligned starts -> a second gather launch runs without a host round trip. The
 * period is the lag mgx_tempo_device writes: librosa's round(60 frame_rate / bpm) with bpm = 60 frame_rate / lag. The
 * reference snapshot has no counterpart, so the definition is stated here in full. Like the statistics, the deltas,
 * the flux, the peaks, the chroma and the tempo it is no feature: MGX_NUM_FEATURES, the name table and every struct
 * above are as they were.
 *
 * The tables (mgx_beat_tables; host only, no device is touched; the caller's, as chroma's bank and the tempogram's
 * window are). P = max_period, 1 .. MGX_BEAT_MAX_PERIOD; tightness finite and > 0 (librosa: 100).
 *   gauss: (P + 1)(P + 2) / 2 float32. Entry p (p + 1) / 2 + k, 1 <= p <= P, k = 0 .. p, is exp(-0.5 (32 k / p)^2),
 *     formed in float64 and rounded once to float32; entry 0 is 1. Underflow to +0 is kept.
 *   penalty: (P + 1)^2 float64. Entry p^2 + d, d = 0 .. 2 p, is -tightness (ln(d / p))^2 for lo(p) <= d <= 2 p -- one
 *     division, one log, one square, one product, in that order -- and -Infinity for d < lo(p) and for p = 0.
 *   lo(p) is p / 2 rounded to the nearest integer, ties to even, and at least 1 (h = p div 2; if p is odd,
 *     h += h & 1; lo = max(1, h)): librosa's np.round(period / 2).
 *
 * The operator. A signal owns rows [a, b) of a one-column envelope x of num_frames values, float32 or float64, taken
 * as float64; n = b - a; p is the signal's entry of `period`. A signal has no beats when n < 2, p = 0 or p > P, and
 * wherever the steps below say so. (local_score and cum_score are +0 in the rows of a signal that stops before
 * step 3, and the values of steps 3 and 5 otherwise.)
 *
 *   1. Scale. 64 partials start at +0; for i = 0 .. n - 1 ascending, P[i mod 64] += x(a + i); then P[l] += P[l + h]
 *      for l < h, with h = 32, 16, .., 1. S = P[0], mean = S / n. Q is formed the same way from e e with
 *      e = x - mean, the product rounded and then added. sd = sqrt(Q / (n - 1)), one correctly rounded division and
 *      one correctly rounded root. No beats unless sd > 0 and sd is finite (so none with a NaN or infinite row).
 *   2. Normalise. xn(t) = x(t) / sd in float64, rounded once to float32; outside [a, b), xn~ is +0.
 *   3. Local score. ls(t) starts at +0; for k = -p .. p ascending, ls(t) += gauss(p, |k|) xn~(t + k): the product of
 *      two float32 values is exact in float64, each addition is rounded once. (The terms outside [a, b) add +0 to a
 *      sum that is never -0, so they may be skipped. |xn| stays near sqrt(n) at most, so it is finite, and a weight
 *      that underflowed to +0 adds a signed zero likewise.)
 *   4. Start. lsmax is a scan of ls over [a, b) from -Infinity with `>`; thr = 0.01 lsmax; t0 is the first t for
 *      which ls(t) < thr is false, or b.
 *   5. Recurrence. For t = a .. b - 1 ascending: best = -Infinity, arg = none; for d = 2 p down to lo(p):
 *      c = penalty(p, d) + C~(t - d), C~(u) = +0 for u < a; if c > best then best = c, arg = d (on a tie the larger d
 *      wins, a NaN never wins). C(t) = ls(t) + best. B(t) = t - arg if t >= t0, arg exists and t - arg >= a; else none.
 *   6. Tail. M(t), a local maximum: for a < t < b - 1, C(t) > C(t - 1) and C(t) >= C(t + 1); M(a) is false; M(b - 1) is
 *      C(b - 1) > C(b - 2). Of the m values C(t) with M(t) in ascending order v (m = 0: no beats), med = v[(m - 1) / 2]
 *      for odd m and (v[m / 2 - 1] + v[m / 2]) 0.5 for even m. tail is the largest t with M(t) and 2 C(t) > med; none:
 *      no beats.
 *   7. Chain. b_0 = tail, b_(i+1) = B(b_i) until none: K rows.
 *   8. Trim. s_i = (0.5 ls(the earlier neighbour in the chain) + ls(b_i)) + 0.5 ls(the later neighbour), a missing
 *      neighbour contributing +0. trim 0: thr = +0. trim 1: R starts at +0 and over the chain in the order of step 7
 *      (descending rows) R += s s, the product rounded and then added; thr = 0.5 sqrt(R / K). A chain row is valid if
 *      s_i > thr; the beats are the chain rows between the lowest and the highest valid row, inclusive; none valid:
 *      no beats.
 *
 * Rows of no signal are never beats and are never written. No atomics: every call below, a repeated call, a graph
 * replay and any grid give the same values. */
#define MGX_BEAT_MAX_PERIOD 1023
typedef struct mgx_beat_params {
  uint32_t struct_size;  /* = sizeof(mgx_beat_params), 16; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t max_period;   /* P, 1 .. MGX_BEAT_MAX_PERIOD: the tables' size; 1023 */
  uint32_t trim;         /* 0 or 1; 1 */
  uint32_t reserved;
} mgx_beat_params;
void mgx_beat_params_init(mgx_beat_params* params);
/* MGX_E_INVALID_ARGUMENT: max_period outside 1 .. MGX_BEAT_MAX_PERIOD, a tightness that is not finite or not
 * positive, NULL gauss or penalty. */
int mgx_beat_tables(uint32_t max_period, double tightness, float* gauss /* (P + 1)(P + 2) / 2 */,
                    double* penalty /* (P + 1)^2 */);
/* The bytes mgx_beats_device works in: a multiple of 256, non-decreasing in both arguments (the picker's bitmaps,
 * two doubles and a back link per row, three words per signal). Host only. */
int mgx_beats_workspace_bytes(uint64_t num_frames, uint64_t num_signals, uint64_t* bytes);

/* The tracker on device arrays; no plan: asynchronous on `stream`, no allocation, no host-side state, capturable.
 * Every pointer is a device pointer. envelope_f64: 0 float32, 1 float64. S is num_signals, or 1 when frame_offsets
 * is NULL and num_signals is 0: one signal [0, num_frames). period: S uint32 (the lag array of mgx_tempo_device).
 * gauss and penalty: mgx_beat_tables of params->max_period, on the device. local_score, cum_score: optional,
 * num_frames doubles each, rows of no signal untouched. The table is read as mgx_peaks_device reads it, and `out` has
 * the picker's exact semantics: the true counts in peak_offsets, the first min(total, capacity) rows in peaks,
 * peak_starts from starts, mask 1 on a beat and 0 on another row of a signal. num_frames = 0 writes peak_offsets (all
 * 0) and nothing else.
 * MGX_E_INVALID_ARGUMENT before any launch: a bad struct_size in either struct, max_period outside 1 ..
 * MGX_BEAT_MAX_PERIOD, trim > 1, envelope_f64 > 1, NULL period, gauss or penalty, mask, peak_offsets and peaks all
 * NULL, peaks set with capacity 0, peak_starts without starts or without peaks, num_signals > 0 with NULL
 * frame_offsets, NULL envelope with num_frames > 0, a workspace smaller than mgx_beats_workspace_bytes or not
 * 256-byte aligned. */
int mgx_beats_device(const void* envelope, uint64_t num_frames, uint32_t envelope_f64, const uint64_t* frame_offsets,
                     uint64_t num_signals, const uint32_t* period, const mgx_beat_params* params, const float* gauss,
                     const double* penalty, double* local_score, double* cum_score, const mgx_peak_outputs* out,
                     void* workspace, uint64_t workspace_bytes, void* stream);

/* Host pointers throughout: mgx_tempo_host's route (the flux of the one request `flux`, its tempogram pooled per
 * clip, the pick under `prior`) with the tracker behind it. The flux column and the lags stay on the device, and the
 * lag array is handed to the tracker as `period`; the tables (mgx_beat_tables of params->max_period) are uploaded once
 * per call. flux->per_frame and flux->summary are honoured as there. Only lag (S uint32, optional), peak_offsets
 * (S + 1, non-NULL: the true counts), the first min(total, capacity) beats (rows of the whole array, ascending; peaks
 * NULL with capacity 0 for the counts alone) and what the request names cross back. The result equals
 * mgx_beats_device on the column and the lags the separate host calls return, wherever the chunks end.
 * MGX_E_INVALID_ARGUMENT: tempo->num_lags - 1 > params->max_period (a lag the tables do not hold), NULL prior or
 * tables, num_signals = 0, and every refusal of mgx_tempo_host and mgx_onsets_host about the arguments they share. */
int mgx_beats_host(mgx_plan* plan, const float* samples, uint64_t num_samples, const uint64_t* starts,
                   uint64_t num_frames, const uint64_t* frame_offsets, uint64_t num_signals,
                   const mgx_flux_request* flux, const mgx_tempo_params* tempo, const float* window, const double* prior,
                   const mgx_beat_params* params, const float* gauss, const double* penalty, uint32_t* lag,
                   uint64_t* peak_offsets, uint64_t* peaks, uint64_t capacity);

/* ---- HPSS: the median-filter harmonic / percussive split of a clip's spectra ---------------------------
 * Replaces, in a host application, the two median filters over the amplitude rows after they were copied back and
 * the masks formed from them (Fitzgerald's median-filtering separation: librosa.decompose.hpss,
 * librosa.effects.harmonic / percussive), and the upload of the two arrays that follows: onset, tempo and beat work
 * runs on the percussive part, chroma on the harmonic part. The reference snapshot has no counterpart. Like the
 * statistics, the deltas, the flux, the peaks, the chroma, the tempo and the beats it is no feature:
 * MGX_NUM_FEATURES, the name table and every struct above are as they were.
 *
 * A signal owns rows [a, b), n = b - a, of an array of num_frames rows x cols float32 columns (row-major). The
 * parameters are a time kernel Kt and a frequency kernel Kf, both odd and 1 .. MGX_HPSS_MAX_KERNEL; ht = Kt div 2,
 * hf = Kf div 2.
 *
 * Order. Values are compared by the IEEE total order of their bit patterns, through the order-preserving key the
 * beat tracker's selection uses: all bits of a negative value flipped, the sign bit of a non-negative one set,
 * compared as unsigned. So -0 < +0, and a NaN with a clear sign bit sorts above +Infinity (one with the sign bit set
 * below -Infinity). The median of an odd window is therefore always one element of the window, bit for bit (a NaN's
 * payload included), and a lone NaN or overflowed amplitude in a window does not become the median.
 *
 * Reflection. An index u outside [0, m) is taken at r(u, m): q = u mod 2m, taken in [0, 2m); r = q if q < m, else
 * 2m - 1 - q. This is the half-sample symmetric extension d c b a | a b c d | d c b a, repeated as often as the
 * window needs (a clip of 2 rows under Kt = 31).
 *
 *   H(t, k) = the median of x(a + r(t - a + j, n), k), j = -ht .. ht     along time, inside the row's own clip only
 *   P(t, k) = the median of x(t, r(k + j, cols)),      j = -hf .. hf     along frequency, inside the row
 *
 * MGX_HPSS_MEDIANS: the two outputs are H and P themselves (the building block of librosa.decompose.nn_filter-style
 * work).
 * MGX_HPSS_SOFT1, MGX_HPSS_SOFT2: the soft masks of power p = 1, 2. Values are taken as float64 (a float32 converts
 * exactly); the margins mh, mp are float32, finite and >= 1. For the harmonic output: A = |H|; R = |P| mh (the
 * product of two float32 is exact); hp = A^p, rp = R^p (for p = 2 one multiplication each, rounded once; A A is
 * exact); den = hp + rp, rounded once, never fused; if den == 0 (both medians are zero) the mask is 0.5 when mh == 1
 * and mp == 1, else 0 (librosa's split_zeros); otherwise mask = hp / den, one correctly rounded float64 division;
 * y = x(t, k) mask, rounded once in float64 and then once to float32. The percussive output is the same with the
 * roles swapped: A = |P|, R = |H| mp.
 * MGX_HPSS_HARD: librosa's power = inf. The harmonic output is x where |H| > |P| mh and +0 elsewhere, the percussive
 * one x where |P| > |H| mp and +0 elsewhere; the comparison is the IEEE one, so a NaN median gives +0.
 * Non-finite values follow IEEE: an infinite median gives Inf / Inf = NaN in its own element.
 *
 * Differences from librosa: its division of both terms by max(X, R) is dropped -- float64 squares of float32 values
 * neither overflow nor underflow, so the zero rule is an exact zero and no comparison with `tiny`; and the arithmetic
 * is float64 with one final rounding, where librosa works in the array's float32.
 * With this order and reflection a numpy statement (tests/hpss_ref.py) equals scipy.ndimage.median_filter(...,
 * mode='reflect') bit for bit on finite non-negative input along both axes for every n <= 19 and odd K <= 63, except
 * for a few cases with K div 2 >= 4 n, where scipy's far extension of a 2-, 4- or 6-row input departs from a periodic
 * reflection. The definition is the formula above, not scipy.
 *
 * An empty signal writes nothing; rows that belong to no signal are not written. A value is a function of its own
 * signal's rows alone: no atomics, and the same bits from every call below, from a repeated call, from a graph replay
 * and from any grid. */
typedef enum mgx_hpss_mode {
  MGX_HPSS_MEDIANS = 0,
  MGX_HPSS_SOFT1 = 1,
  MGX_HPSS_SOFT2 = 2,
  MGX_HPSS_HARD = 3,
  MGX_NUM_HPSS_MODES = 4
} mgx_hpss_mode;
#define MGX_HPSS_MAX_KERNEL 31
/* The kernel's tile (mgx_hpss_tile reports it): a clip whose length straddles MGX_HPSS_TILE_ROWS, or an array whose
 * width straddles MGX_HPSS_TILE_COLS, takes another path through it. Not part of the definition. */
#define MGX_HPSS_TILE_ROWS 64
#define MGX_HPSS_TILE_COLS 64
typedef struct mgx_hpss_params {
  uint32_t struct_size;      /* = sizeof(mgx_hpss_params), 24; anything else: MGX_E_INVALID_ARGUMENT */
  uint32_t kernel_time, kernel_freq;   /* Kt, Kf; 31, 31 */
  uint32_t mode;             /* mgx_hpss_mode; MGX_HPSS_SOFT2 */
  float margin_harmonic, margin_percussive;   /* 1, 1 */
} mgx_hpss_params;
void mgx_hpss_params_init(mgx_hpss_params* params);
void mgx_hpss_tile(uint32_t* tile_rows, uint32_t* tile_cols);  /* either may be NULL */

/* The operator on device arrays; no plan: asynchronous on `stream`, no allocation, no workspace, no host-side
 * state, capturable; one launch that reads the array once. rows, harmonic, percussive: num_frames x cols float32;
 * either output may be NULL, not both. The table is read as mgx_delta_device reads it, every entry limited to
 * num_frames: a non-decreasing one gives the definition above, any other gives unspecified values and no access
 * outside the arrays. NULL with num_signals = 0 means one signal [0, num_frames).
 * MGX_E_INVALID_ARGUMENT before any launch: NULL params or a bad struct_size, an even kernel or one outside 1 ..
 * MGX_HPSS_MAX_KERNEL, mode >= MGX_NUM_HPSS_MODES, a margin that is NaN, infinite or below 1, cols = 0, both outputs
 * NULL, an output equal to rows or to the other output (halos are read: the operator cannot run in place),
 * num_signals > 0 with NULL frame_offsets, NULL rows with num_frames > 0. num_frames = 0 returns MGX_OK and writes
 * nothing. */
int mgx_hpss_device(const float* rows, uint64_t num_frames, uint32_t cols,
                    const uint64_t* frame_offsets, uint64_t num_signals,
                    const mgx_hpss_params* params,
                    float* harmonic, float* percussive, void* stream);

/* Host pointers throughout: mgx_extract_gather_host with the amplitude spectrum as a field that does not cross back.
 * A time median reaches across chunk ends, so each chunk's amplitude rows are copied, device to device, into a
 * plan-owned num_frames x N/2 array that lasts as long as the call (as the delta host call keeps its rows; grown on
 * demand, freed at mgx_plan_destroy; MGX_E_OUT_OF_MEMORY when the device has no room). After the last chunk
 * mgx_hpss_device runs once over it; the harmonic and percussive arrays are plan-owned too, and only those that
 * something consumes are allocated. Then mgx_chroma_device runs on the harmonic rows (harmonic_chroma) and
 * mgx_flux_device on the percussive rows (percussive_flux, whose field must be MGX_AMPLITUDE_SPECTRUM); per_frame and
 * summary of either request are written and pooled exactly as mgx_chroma_host and mgx_summarize_flux_host write and
 * pool them. harmonic, percussive: num_frames x N/2 floats each, or NULL; of these the rows of the signals alone are
 * written, as the operator writes them (every row when frame_offsets is NULL with num_signals = 0). The result equals
 * the composition of the device operators on the rows mgx_extract_gather_host returns, bit for bit, wherever the
 * chunks end. Only what the caller names crosses back.
 * MGX_E_INVALID_ARGUMENT: all four outputs NULL, NULL params, and every refusal of mgx_hpss_device, mgx_chroma_host
 * and the flux request of mgx_summarize_flux_host about the arguments they share (a request with both pointers NULL, a
 * summary with num_signals = 0); a flux field other than MGX_AMPLITUDE_SPECTRUM is MGX_E_UNSUPPORTED. */
int mgx_hpss_host(mgx_plan* plan, const float* samples, uint64_t num_samples,
                  const uint64_t* starts, uint64_t num_frames,
                  const uint64_t* frame_offsets, uint64_t num_signals,
                  const mgx_hpss_params* params,
                  const mgx_chroma_request* harmonic_chroma,   /* or NULL */
                  const mgx_flux_request* percussive_flux,     /* or NULL; field must be MGX_AMPLITUDE_SPECTRUM */
                  float* harmonic, float* percussive);         /* num_frames x N/2 each, or NULL */

/* ---- Multi-device groups -------------------------------
 * Replaces nothing in the reference (single-threaded browser code); it exists because
 * buffers are independent (src/meyda.js:69-91 keeps no cross-buffer state), so a batch
 * is cut into contiguous shards, one per device, each extracted by that device's plan
 * (the plan of `new Meyda(...)`, src/meyda.js:17-97), and the per-frame feature records
 * are gathered to the root device (rank 0) over xGMI by RCCL point-to-point transfers.
 * The gather is chunked: chunk i of every shard is sent while chunk i+1 is extracted.
 * RCCL (librccl.so.1, or $MGX_RCCL_LIB) is loaded when a group of more than one rank is
 * created; a one-rank group needs no RCCL. */
typedef struct mgx_group mgx_group;

#define MGX_COMM_ID_BYTES 128  /* an RCCL unique id (ncclUniqueId) */

/* Output selection of a group extraction (every rank passes the same mask). */
#define MGX_OUT_SCALAR(i) (1u << (i))       /* i < MGX_NUM_SCALARS */
#define MGX_OUT_LOUDNESS_SPECIFIC (1u << 13)
#define MGX_OUT_MFCC (1u << 14)
#define MGX_OUT_AMPLITUDE_SPECTRUM (1u << 15)
#define MGX_OUT_POWER_SPECTRUM (1u << 16)
#define MGX_OUT_COMPLEX_SPECTRUM (1u << 17)   /* real and imag */
#define MGX_OUT_ALL_MASK ((1u << 18) - 1)

/* Contiguous shard [*start, *start + *count) of `total` frames for `rank` of `nranks`:
 * the first total % nranks ranks get one frame more. Host only. */
int mgx_shard_range(uint64_t total, uint32_t nranks, uint32_t rank, uint64_t* start, uint64_t* count);

/* Byte offsets of the outputs of `num_frames` frames packed into one transfer buffer
 * (structure of arrays, each array 256-byte aligned, in mgx_outputs order: 13 scalars,
 * loudness_specific, mfcc, amplitude, power, complex real, complex imag). offsets[i] is
 * the offset of field i (MGX_OUT_* bit i; the complex field has two arrays: offsets[17]
 * real, offsets[18] imag), or UINT64_MAX when not in `mask`. Returns the total bytes.
 * Host only; the root unpacks each peer's chunk with the same arithmetic. */
uint64_t mgx_packed_layout(const mgx_plan_desc* desc, uint32_t mask, uint64_t num_frames, uint64_t offsets[19]);

/* Single process, several devices (RCCL ncclCommInitAll): devices[0] is the root. */
int mgx_group_create(const mgx_plan_desc* desc, const int32_t* devices, uint32_t num_devices, mgx_group** out);

/* One process per device (e.g. torchrun): rank 0 calls mgx_comm_unique_id and the caller
 * broadcasts the bytes; every rank then calls mgx_group_create_rank with its rank.
 * desc->device is this rank's device. Rank 0 is the root.
 * Test transport across processes: with MGX_GROUP_TRANSPORT=ipc in the environment of every
 * rank, the id names a POSIX shared-memory mailbox instead of an RCCL communicator, and each
 * peer chunk reaches the root through hipIpcGetMemHandle / hipIpcOpenMemHandle of the peer's
 * transfer buffer (a device copy on the root's communication stream, handed over through the
 * mailbox's per-slot sequence numbers) -- the multi-rank data path across a process boundary,
 * runnable with every rank on one GPU (RCCL refuses that). $MGX_IPC_TIMEOUT_S (default 60)
 * bounds each wait for a peer; a missing peer is an MGX_E_DEVICE error, not a hang. */
int mgx_comm_unique_id(void* id, uint64_t id_bytes);
int mgx_group_create_rank(const mgx_plan_desc* desc, const void* unique_id, uint32_t nranks, uint32_t rank,
                          mgx_group** out);
/* Test transport: nranks ranks in this process, all on desc->device, whose chunk transfers
 * are device copies into the root's staging slots instead of RCCL messages. Everything
 * else -- shards, chunks, transfer slots, the two compute streams, the root's unpack -- is
 * the multi-device path's own code, so one GPU can check the gather byte for byte. */
int mgx_group_create_loopback(const mgx_plan_desc* desc, uint32_t nranks, mgx_group** out);
/* The same test group with the RCCL transport: the root holds a one-rank RCCL
 * communicator on desc->device, and each peer chunk crosses as an ncclSend to self matched
 * by an ncclRecv from self (one ncclGroupStart/End each) on the root's communication
 * stream -- the RCCL calls, message sizes, slot ordering and unpack of the multi-rank
 * path, runnable on one GPU (RCCL refuses two ranks on one device). */
int mgx_group_create_loopback_rccl(const mgx_plan_desc* desc, uint32_t nranks, mgx_group** out);
int mgx_group_destroy(mgx_group* group);
/* Ranks of the group, and the ranks this process drives (num_local = 1 per process, or
 * all of them in single-process mode, first_local = their first rank). */
int mgx_group_info(const mgx_group* group, uint32_t* nranks, uint32_t* first_local, uint32_t* num_local);
/* What the RCCL communicator of this process's first local rank reports: ranks in the
 * communicator (ncclCommCount), this rank in it (ncclCommUserRank) and its device
 * (ncclCommCuDevice); all -1 when the group has no communicator (one rank, or device copies).
 * MGX_E_UNSUPPORTED when the loaded RCCL lacks those three queries (the data path does not
 * need them). */
int mgx_group_comm_info(const mgx_group* group, int32_t* comm_ranks, int32_t* comm_rank, int32_t* comm_device);

/* Device-resident batch. frames[i]: device pointer of the shard of local rank
 * first_local + i (on that rank's device); counts: frames of every rank (nranks
 * entries, the same on every rank; shard r holds global frames [sum counts[<r],
 * + counts[r])). root_out: device pointers on the root device sized for sum(counts)
 * frames (read on the root only; may be NULL elsewhere); every field in `mask` must be
 * non-NULL there. num_chunks: pipeline depth (0 = automatic). streams: NULL for the
 * group's own streams, else streams[i] is local rank i's stream (a NULL entry is that
 * device's default stream): the work is ordered after what is enqueued on it, and it
 * waits for the work's completion (gather included). Asynchronous. */
int mgx_group_extract_device(mgx_group* group, const float* const* frames, const uint64_t* counts,
                             const mgx_outputs* root_out, uint32_t mask, uint32_t num_chunks,
                             void* const* streams);

/* Host batch in, host outputs (single-process groups): the frames are cut into one
 * shard per device (mgx_shard_range), copied to the devices in parallel, extracted,
 * gathered to the root device by RCCL and copied back. Output layout as mgx_extract_host. */
int mgx_group_extract_host(mgx_group* group, const float* frames, uint64_t num_frames, const mgx_outputs* outputs);

int mgx_is_power_of_two(double n);           /* src/utils.js:13-19 */
int mgx_feature_index(const char* name);     /* -1 if unknown */
const char* mgx_feature_name(int feature);   /* NULL if out of range */
int mgx_feature_info(int feature);           /* mgx_info_type, or -1 */
int mgx_device_count(int* count);
int mgx_abi_version(void);
const char* mgx_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* MEYDA_GPU_H */
