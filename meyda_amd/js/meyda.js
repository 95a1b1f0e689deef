'use strict';
// Meyda-compatible JavaScript facade over the MI355X engine.
//
// Same surface as the reference class (src/meyda.js:15-263):
//   new Meyda(audioContext, source, bufferSize, callback)      src/meyda.js:17-97
//   get(feature | features[])                                  :244-261
//   start(features) / stop()                                   :233-241
//   setSource(source)                                          :229-231
//   featureInfo, windowingFunction, hanning, hamming, barkScale, signal
// plus, for the batched engine:
//   process(signal)                 push one buffer (what onaudioprocess does, :69-91)
//   getBatch(features, frames)      frames: Float32Array(F * bufferSize) -> SoA typed arrays
//   getBatchAsync(features, frames) same, off the JS thread (napi_async_work)
//   getBatchWav(features, wavBytes[, channel[, hopSize]]) / getBatchWavAsync(...)
//                                   every full buffer of a .wav file (RIFF walk in C, raw PCM
//                                   decoded on the device: decodeAudioData's scaling); with hopSize,
//                                   the buffers that start every hopSize samples
//   getBatchSignal(features, samples, hopSize) / getBatchSignalAsync(...)
//                                   samples: one contiguous Float32Array; the overlapping buffers
//                                   that start every hopSize samples (later Meyda's hopSize), read
//                                   in place on the device, a trailing partial buffer dropped
//   Meyda.signalFrames(numSamples, bufferSize, hopSize)
//                                   how many buffers that is: (numSamples - bufferSize) / hopSize + 1
//   getBatchGather(features, samples, starts) / getBatchGatherAsync(...)
//                                   buffer f is samples [starts[f], starts[f] + bufferSize): any order,
//                                   repeats and overlaps allowed, one launch for all of them
//   getBatchSignals(features, signals, hopSize) / getBatchSignalsAsync(...)
//                                   signals: an array of Float32Arrays (a corpus); every signal's buffers
//                                   in one launch, none across two signals; getBatch's result plus
//                                   frameOffsets (signal s: rows frameOffsets[s] .. frameOffsets[s + 1])
//   getSignalSummaries(features, signals, hopSize[, {deltaWidth, deltaOrder, flux}]) / getSignalSummariesAsync(...)
//                                   getBatchSignals' signals pooled per signal on the device: per feature
//                                   {mean, variance, min, max}, Float64Arrays of signals x width, plus frameOffsets
//   getSignalOnsets(signals, hopSize, {feature, mode, lag, preMax, postMax, preAvg, postAvg, delta, wait, envelope})
//   / getSignalOnsetsAsync(...)     the onsets of every signal: the peaks of a feature's spectral flux, picked on
//                                   the device within each signal; {frameOffsets, onsetOffsets, onsets[, envelope]}
//   getSignalChroma(signals, hopSize[, {weights, numChroma, a440, centerOctave, octaveWidth, baseC, norm, summary}])
//   / getSignalChromaAsync(...)     the pitch-class profile of every buffer of every signal (later Meyda's chroma),
//                                   computed on the device from spectra that stay there; {chroma, numChroma,
//                                   frameOffsets[, summaries]}
//   Meyda.chromaFilterBank(bufferSize, sampleRate[, options])
//                                   the numChroma x bufferSize / 2 chroma filter bank (host only)
//   getSignalHpss(signals, hopSize, {kernelSize | [kernelTime, kernelFreq], power: 1 | 2 | Infinity,
//                                    margin | [marginHarmonic, marginPercussive], chroma: {getSignalChroma's options},
//                                    flux: {mode, lag, summary}, harmonic, percussive}) / getSignalHpssAsync(...)
//                                   the median-filter harmonic / percussive split of every signal's amplitude spectra
//                                   (librosa.decompose.hpss), on the device from spectra that stay there: the chroma of
//                                   the harmonic part, the flux of the percussive part (the onset envelope), the two
//                                   parts themselves where asked for; {frameOffsets[, harmonic][, percussive][, chroma,
//                                   numChroma[, chromaSummaries]][, flux[, fluxSummaries]]}
//   getSignalTempo(signals, {hopSize, feature, mode, lag, winLength, numLags, norm, gain, startBpm, stdOctaves,
//                            maxBpm, window, prior, mean, envelope}) / getSignalTempoAsync(...)
//                                   the tempo of every signal: the autocorrelation tempogram of a feature's spectral
//                                   flux, pooled per signal, and the lag a tempo prior picks, all on the device;
//                                   {frameOffsets, lag, bpm, numLags[, mean][, envelope]}
//   Meyda.tempogramWindow(winLength), Meyda.tempoPrior(frameRate, numLags[, {startBpm, stdOctaves, maxBpm}])
//                                   the periodic Hann window and the log-normal tempo prior (host only)
//   getSignalBeats(signals, {getSignalTempo's options but mean, tightness, trim, maxPeriod}) / getSignalBeatsAsync(...)
//                                   the beats of every signal: getSignalTempo's lag, and the buffers a dynamic
//                                   programme places the beats on at that period, all on the device; only the lags
//                                   and the beat lists cross back
//   Meyda.beatTables(maxPeriod[, tightness])
//                                   the tracker's tables {gauss, penalty} (host only)
//   Meyda.signalsFrameStarts(lengths, bufferSize, hopSize)
//                                   {starts, frameOffsets} of signals stored one after another
//   Meyda.readWav(wavBytes)         the header: {pcmFormat, channels, sampleRate, sampleFrames, ...}
//   'melBands'                      a feature name beyond the snapshot's 18 (later Meyda's melBands): the
//                                   log mel band energies the MFCC is the DCT of (mfcc.js:53-65), a
//                                   Float32Array(options.numMelBands) per buffer; in get(), start() and
//                                   every getBatch* form, not with options.devices
//   flush()                         deliver buffered callbacks now (options.batchFrames > 1)
//   options.devices = [0, 1, ...]   shard batches over several GPUs; the feature records are
//                                   gathered to the first one by RCCL (one plan per device)
//   options.asyncPlans = 2          plans per window that async batch jobs run on; more jobs
//                                   queue on them
//
// Streaming (start/stop, src/meyda.js:69-91,233-241): with options.batchFrames = K > 1
// the buffers pushed by process() are queued and extracted K at a time in one launch;
// the callback still runs once per buffer, in order, with that buffer's features
// (latency of up to K buffers for K-fold fewer launches). stop() flushes the queue.
//
// Every built-in feature is computed by libmeyda_gpu.so through the N-API addon.
// Differences from the snapshot (documented in INTEGRATION.md): the FFT runs per
// buffer (the snapshot never transforms, src/meyda.js:79-84; opt back in with
// {mode: 'literal'}), all 18 extractors are registered (src/extractors/index.js
// enables only loudness), the callback works (src/meyda.js:87 references an
// undefined global), and get() returns fresh arrays rather than internal buffers.
const path = require('path');

// (Loading the module changes nothing outside it, like the reference's constructor: the HIP runtime's
// settings are the application's. For the real-time path, HIP_FORCE_DEV_KERNARG=0 in the environment
// that starts the process keeps kernel arguments in host memory -- a ~1.4 us shorter launch call, ~0.6 us
// per one-frame call end to end; INTEGRATION.md, profiles/r05_inline_frame.txt.)
const addon = require(process.env.MEYDA_AMD_ADDON ||
  path.join(__dirname, '..', 'addon', 'meyda_napi.node'));
const FEATURE_INFO = require('./feature-info');

const GPU_FEATURES = new Set(['rms', 'energy', 'zcr', 'spectralCentroid', 'spectralFlatness',
  'spectralSlope', 'spectralRolloff', 'spectralSpread', 'spectralSkewness', 'spectralKurtosis',
  'perceptualSpread', 'perceptualSharpness', 'loudness', 'mfcc', 'amplitudeSpectrum',
  'powerSpectrum', 'complexSpectrum', 'melBands']);

// src/utils.js:13-19
function isPowerOfTwo(num) {
  while (((num % 2) === 0) && num > 1) num /= 2;
  return (num == 1); // eslint-disable-line eqeqeq
}

class Meyda {
  constructor(audioContext, src, bufSize, callback, options) {
    // src/meyda.js:20-26: validated in this order, so `bufSize || 256` is unreachable
    if (!isPowerOfTwo(bufSize)) {
      throw new Error('Buffer size is not a power of two: Meyda will not run.');
    }
    if (!audioContext) {
      throw new Error("AudioContext wasn't specified: Meyda will not run.");
    }
    const bufferSize = bufSize || 256;
    this.audioContext = audioContext;
    this.bufferSize = bufferSize;
    this.sampleRate = audioContext.sampleRate;
    this.options = Object.assign({
      precision: 'faithful', mode: 'per_buffer_fft', numMelBands: 26, numMfccCoeffs: 13, device: 0,
      batchFrames: 1,
    }, options || {});
    this._ring = null;        // queued buffers (batchFrames > 1)
    this._flushing = null;    // the ring whose frames a flush is delivering
    this._layouts = new Map(); // extractViews' output layouts, per (fields, frames)
    this._ringCount = 0;
    this.featureExtractors = {}; // user plugins: fn(bufferSize, m) or {process(signal)}
    this.EXTRACTION_STARTED = false;
    this._featuresToExtract = null;
    this._callback = callback;
    this.windowingFunction = 'hanning';
    const t = addon.hostTables({ bufferSize, sampleRate: this.sampleRate,
      numMelBands: this.options.numMelBands, numMfccCoeffs: this.options.numMfccCoeffs });
    this.barkScale = t.barkScale;
    this.hanning = t.hanning;
    this.hamming = t.hamming;
    this.featureInfo = Object.assign({}, FEATURE_INFO);
    this.signal = null;
    this._plans = {};       // streaming / sync plan per window
    this._asyncPlans = {};  // per window: plans that async batch jobs run on (never the streaming one)
    this._frame = null; // results of the current buffer, filled lazily by get()
    // Web Audio wiring when the context provides it (src/meyda.js:67-94). One node per
    // instance (the reference stored it on a window global).
    if (typeof audioContext.createScriptProcessor === 'function') {
      this.spn = audioContext.createScriptProcessor(bufferSize, 1, 1);
      this.spn.onaudioprocess = (e) => this.process(e.inputBuffer.getChannelData(0));
      if (typeof this.spn.connect === 'function' && audioContext.destination) {
        this.spn.connect(audioContext.destination);
      }
      if (src && typeof src.connect === 'function') src.connect(this.spn, 0, 0);
    }
  }

  // `signal`: the current buffer (src/meyda.js:70). In a batched callback it is a view of the queued
  // frames, made on first read.
  get signal() {
    if (this._sigBatch) {
      const i = this._sigIndex, N = this.bufferSize;
      this._sig = this._sigBatch.subarray(i * N, i * N + N);
      this._sigBatch = null;
    }
    return this._sig;
  }

  set signal(v) {
    this._sig = v;
    this._sigBatch = null;
  }

  _window() {
    const w = this.windowingFunction;
    if (w !== 'hanning' && w !== 'hamming') {
      throw new TypeError('unknown windowingFunction "' + w + '"');
    }
    return w;
  }

  _newPlan(w) {
    return addon.createPlan({
      bufferSize: this.bufferSize, sampleRate: this.sampleRate, windowingFunction: w,
      precision: this.options.precision, mode: this.options.mode,
      numMelBands: this.options.numMelBands, numMfccCoeffs: this.options.numMfccCoeffs,
      device: this.options.device, scalarF64: 1,
      // options.mfccReferenceOrder: mel sums, log and DCT in mfcc.js's own order (bit-identical MFCC)
      mfccReferenceOrder: this.options.mfccReferenceOrder ? 1 : 0,
      // options.resident: one-buffer calls (the per-buffer process()/get() path) served by a workgroup that
      // stays on the device between buffers instead of one launch per buffer (include/meyda_gpu.h
      // MGX_FLAG_RESIDENT); one device, faithful per-buffer plans without mfccReferenceOrder
      resident: this.options.resident && !Array.isArray(this.options.devices) ? 1 : 0,
      // options.devices = [d0, d1, ...]: every batch is sharded over the devices and the
      // per-frame features are gathered to d0 over xGMI (RCCL), include/meyda_gpu.h mgx_group_*
      ...(Array.isArray(this.options.devices) ? { devices: this.options.devices } : {}),
    });
  }

  // One plan per window type, created on first use (windowingFunction may change at
  // runtime as in the reference, src/meyda.js:41,76,164). process()/get()/getBatch() run on it.
  _plan() {
    const w = this._window();
    if (!this._plans[w]) this._plans[w] = this._newPlan(w);
    return this._plans[w];
  }

  // Async batch jobs own their plan for the whole job (the addon marks it busy), so they
  // never run on the streaming plan: per window, a pool of at most options.asyncPlans plans
  // (default 2; with options.devices each one is a whole device group with its RCCL
  // communicators), so onaudioprocess buffers and a second async batch proceed while a job
  // is in flight. Further jobs queue on the pooled plan with the fewest pending jobs.
  _runAsync(job) {
    const w = this._window();
    const pool = this._asyncPlans[w] || (this._asyncPlans[w] = []);
    const cap = Math.max(1, this.options.asyncPlans | 0 || 2);
    let slot = pool.find((sl) => sl.pending === 0);
    if (!slot && pool.length < cap) {
      slot = { plan: this._newPlan(w), pending: 0, tail: Promise.resolve() };
      pool.push(slot);
    }
    if (!slot) slot = pool.reduce((a, b) => (b.pending < a.pending ? b : a));
    slot.pending++;
    const run = () => job(slot.plan);
    const res = slot.tail.then(run, run);
    const done = () => { slot.pending--; };
    slot.tail = res.then(done, done);
    return res;
  }

  // The per-buffer handler (src/meyda.js:69-91): take the buffer, then deliver the
  // started features to the callback.
  process(signal) {
    if (!(signal instanceof Float32Array)) signal = Float32Array.from(signal);
    if (signal.length !== this.bufferSize) {
      throw new RangeError('buffer length ' + signal.length + ' != bufferSize ' + this.bufferSize);
    }
    this.signal = signal;
    this._frame = null;
    if (typeof this._callback !== 'function' || !this.EXTRACTION_STARTED) return;
    const K = this.options.batchFrames | 0;
    if (K <= 1) {
      this._callback(this.get(this._featuresToExtract));
      return;
    }
    if (!this._ring || this._ring === this._flushing || this._ring.length !== K * this.bufferSize) {
      this._ring = new Float32Array(K * this.bufferSize);
    }
    this._ring.set(signal, this._ringCount * this.bufferSize);
    if (++this._ringCount === K) this.flush();
  }

  // Extract every queued buffer in one launch and run the callback for each, in order.
  flush() {
    const count = this._ringCount;
    if (!count) return;
    this._ringCount = 0;
    const list = this._featuresToExtract;
    const names = typeof list === 'string' ? [list] : Array.prototype.slice.call(list || []);
    const plugins = names.some((n) => this.featureExtractors[n]);
    if (!plugins && names.every((n) => GPU_FEATURES.has(n) || n === 'buffer')) {
      this._flushViews(count, list, names);
      return;
    }
    const gpu = names.filter((n) => GPU_FEATURES.has(n) && !this.featureExtractors[n]);
    if (plugins) gpu.push('amplitudeSpectrum', 'complexSpectrum', 'loudness');
    const N = this.bufferSize;
    const frames = this._ring.slice(0, count * N);
    this._checkNames(gpu);
    const r = gpu.length ? addon.extract(this._plan(), frames, gpu) : {};
    const keep = this.signal;
    for (let i = 0; i < count; i++) {
      const sig = frames.subarray(i * N, (i + 1) * N);
      this.signal = sig;
      this._frame = {};
      for (const n of new Set(gpu)) this._frame[n] = frameValue(n, r, i, N, this.options.numMfccCoeffs, this.options.numMelBands);
      const out = typeof list === 'string' ? this._value(list) : this.get(names);
      this._callback(out);
    }
    this.signal = keep;
    this._frame = null;
  }

  // flush() for built-in features only: one launch, then each callback gets its frame's values as
  // views into the batch's result arrays (numbers, and subarrays where get() returns arrays), built by
  // one compiled object literal per feature list (frameBuilder) instead of per-frame copies and a get()
  // dispatch per buffer. The batch's result arrays are fresh per launch, so a view stays valid after its
  // callback. `signal` is a view of the queued frames, made only if read (the ring is reused by the
  // next batch); 'buffer' is a copy of the frame.
  _flushViews(count, list, names) {
    const N = this.bufferSize, nc = this.options.numMfccCoeffs || 13, nm = this.options.numMelBands || 26;
    const frames = this._ring.subarray(0, count * N);
    this._flushing = this._ring;  // (a process() from a callback starts a new ring: these frames stay put)
    const gpu = Array.from(new Set(names.filter((n) => n !== 'buffer')));
    this._checkNames(gpu);
    const r = gpu.length ? extractViews(this._layouts, this._plan(), frames, gpu, N, nc, nm) : {};
    const keep = this.signal;
    const cb = this._callback;
    const build = frameBuilder(typeof list === 'string' ? null : names, typeof list === 'string' ? list : null);
    for (let i = 0; i < count; i++) {
      this._sigBatch = frames;
      this._sigIndex = i;
      this._frame = null;
      cb(build(r, frames, i, N, nc, nm));
    }
    this._flushing = null;
    this.signal = keep;
    this._frame = null;
  }

  setSource(_src) {
    _src.connect(this.spn);
  }

  start(features) {
    this._featuresToExtract = features;
    this.EXTRACTION_STARTED = true;
  }

  stop() {
    if (this._ringCount) this.flush();  // queued buffers are still delivered
    this._featuresToExtract = null;
    this.EXTRACTION_STARTED = false;
  }

  // src/meyda.js:244-261
  get(feature) {
    if (typeof feature === 'object') {
      const names = Array.prototype.slice.call(feature); // null throws, as feature.length does
      const gpu = [];
      for (let x = 0; x < names.length; x++) {
        const n = names[x];
        if (GPU_FEATURES.has(n) && !this.featureExtractors[n]) gpu.push(n);
      }
      try {  // one launch for all built-in features; a failure resurfaces per feature below
        this._compute(gpu);
      } catch (e) { /* logged per feature, as the reference does */ }
      const results = {};
      for (let x = 0; x < names.length; x++) {
        try {
          results[names[x]] = this._value(names[x]);
        } catch (e) {
          console.error(e);
        }
      }
      return results;
    } else if (typeof feature === 'string') {
      return this._value(feature);
    }
    throw new Error('Invalid Feature Format');
  }

  _signal() {
    return this.signal || new Float32Array(this.bufferSize);
  }

  // Compute the missing GPU features of the current buffer in one launch.
  _compute(names) {
    const fr = this._frame || (this._frame = {});
    const need = [];
    for (let x = 0; x < names.length; x++) if (!(names[x] in fr)) need.push(names[x]);
    if (!need.length) return;
    // (into the layout's scratch buffer: frameValue copies every value out before anything else runs)
    this._checkNames(need);
    const r = extractViews(this._layouts, this._plan(), this._signal(), need, this.bufferSize, this.options.numMfccCoeffs,
      this.options.numMelBands, true);
    for (const n of need) this._frame[n] = frameValue(n, r, 0, this.bufferSize, this.options.numMfccCoeffs, this.options.numMelBands);
  }

  _value(name) {
    const plugin = this.featureExtractors[name];
    if (plugin) return this._runPlugin(plugin);
    const fr = this._frame;
    if (fr && name in fr) return fr[name];  // this buffer's launch computed it
    if (name === 'buffer') return this._signal();
    if (!GPU_FEATURES.has(name)) {
      throw new TypeError("Cannot read property 'process' of undefined (feature '" + name + "')");
    }
    this._compute([name]);
    return this._frame[name];
  }

  // A user extractor sees the same `m` the reference extractors see
  // (SURVEY.md §8(b)): signal, ampSpectrum, complexSpectrum, audioContext, featureExtractors.
  _runPlugin(plugin) {
    if (typeof plugin.process === 'function') return plugin.process(this._signal());
    this._compute(['amplitudeSpectrum', 'complexSpectrum', 'loudness']);
    const m = {
      signal: this._signal(),
      ampSpectrum: this._frame.amplitudeSpectrum,
      complexSpectrum: this._frame.complexSpectrum,
      audioContext: this.audioContext,
      featureExtractors: Object.assign({ loudness: () => this._frame.loudness }, this.featureExtractors),
    };
    return plugin(this.bufferSize, m);
  }

  // Batch API: frames is a Float32Array holding F consecutive buffers.
  getBatch(features, frames) {
    const names = this._checkNames(checkBatchNames(features));
    return addon.extract(this._plan(), toF32(frames), names);
  }

  getBatchAsync(features, frames) {
    const names = this._checkNames(checkBatchNames(features));
    const x = toF32(frames);
    return this._runAsync((plan) => addon.extractAsync(plan, x, names));
  }

  // Every full buffer of a .wav file (Buffer / Uint8Array / ArrayBuffer), channel `channel`; with
  // hopSize, the buffers that start every hopSize samples of that channel.
  getBatchWav(features, wavBytes, channel, hopSize) {
    const names = this._checkNames(checkBatchNames(features));
    if (hopSize === undefined) return addon.extractWav(this._plan(), wavBytes, names, channel | 0);
    const hop = this._checkHop(hopSize);
    return addon.extractWav(this._plan(), wavBytes, names, channel | 0, hop);
  }

  getBatchWavAsync(features, wavBytes, channel, hopSize) {
    const names = this._checkNames(checkBatchNames(features));
    if (hopSize === undefined) return this._runAsync((plan) => addon.extractWavAsync(plan, wavBytes, names, channel | 0));
    const hop = this._checkHop(hopSize);
    return this._runAsync((plan) => addon.extractWavAsync(plan, wavBytes, names, channel | 0, hop));
  }

  // Overlapping buffers of one contiguous signal: buffer f is samples [f hopSize, f hopSize + bufferSize),
  // Meyda.signalFrames(samples.length, bufferSize, hopSize) of them; results as getBatch's.
  getBatchSignal(features, samples, hopSize) {
    const names = this._checkNames(checkBatchNames(features));
    const hop = this._checkHop(hopSize);
    return addon.extractSignal(this._plan(), toF32(samples), hop, names);
  }

  getBatchSignalAsync(features, samples, hopSize) {
    const names = this._checkNames(checkBatchNames(features));
    const hop = this._checkHop(hopSize);
    const x = toF32(samples);
    return this._runAsync((plan) => addon.extractSignalAsync(plan, x, hop, names));
  }

  // Buffers at given sample offsets: buffer f is samples [starts[f], starts[f] + bufferSize) of one
  // Float32Array. starts: an array or typed array of non-negative safe integers, in any order (they may
  // repeat and overlap); one whose buffer leaves the samples is refused. Results as getBatch's.
  getBatchGather(features, samples, starts) {
    const names = this._checkNames(checkBatchNames(features));
    const st = this._checkStarts(starts);
    return addon.extractGather(this._plan(), toF32(samples), st, names);
  }

  getBatchGatherAsync(features, samples, starts) {
    const names = this._checkNames(checkBatchNames(features));
    const st = this._checkStarts(starts);
    const x = toF32(samples);
    return this._runAsync((plan) => addon.extractGatherAsync(plan, x, st, names));
  }

  // Many signals in one call: signals is an array of Float32Arrays, each cut every hopSize samples as
  // getBatchSignal cuts one, no buffer across two signals. getBatch's result object over all the buffers
  // in signal order, with frameOffsets added: signal s's buffers are rows
  // [frameOffsets[s], frameOffsets[s + 1]) of every output.
  getBatchSignals(features, signals, hopSize) {
    const names = this._checkNames(checkBatchNames(features));
    const c = this._concatSignals(signals, hopSize);
    const r = addon.extractGather(this._plan(), c.samples, c.starts, names);
    r.frameOffsets = c.frameOffsets;
    return r;
  }

  getBatchSignalsAsync(features, signals, hopSize) {
    const names = this._checkNames(checkBatchNames(features));
    const c = this._concatSignals(signals, hopSize);
    return this._runAsync((plan) => addon.extractGatherAsync(plan, c.samples, c.starts, names)).then((r) => {
      r.frameOffsets = c.frameOffsets;
      return r;
    });
  }

  // The signals of getBatchSignals pooled per signal on the device: for every feature {mean, variance, min,
  // max}, Float64Arrays of signals.length x width (width: the feature's values per buffer, 1 for a number;
  // signal s at [s width, (s + 1) width)); 'loudness' gives {specific, total}, each such an object. Population
  // variance; a signal without buffers gives NaN. frameOffsets as getBatchSignals returns it. Only the
  // summaries cross back from the device. 'complexSpectrum' and 'buffer' have no summary (TypeError).
  // options {deltaWidth: 2, deltaOrder: 2}: the same statistics of the rows' regression deltas of half-width
  // deltaWidth (1..8) within each signal, and at order 2 of the deltas' deltas (MFCC + delta + delta-delta pooled
  // per clip): the result gains `delta` (and `delta2`), objects of the result's own shape. The deltas of a
  // spectrum are not pooled (the library's error). Without the option the result is as it was.
  // options {flux: [{feature, mode: 'rectified' | 'l1' | 'l2', lag: 1..8, perFrame}]} (up to 4): the spectral flux
  // of 'loudness' (its specific rows), 'mfcc', 'amplitudeSpectrum', 'powerSpectrum' or 'melBands' -- the distance
  // of every buffer's row from the row `lag` buffers before it in the same signal (include/meyda_gpu.h) -- pooled
  // per signal: the result gains `flux`, one object per request with mean, variance, min, max (Float64Arrays of
  // signals.length) and, with perFrame, the onset envelope `perFrame` (a Float32Array, a value per buffer). An
  // options object with flux and no delta key asks for no deltas.
  getSignalSummaries(features, signals, hopSize, options) {
    const names = this._checkNames(checkSummaryNames(features));
    const c = this._concatSignals(signals, hopSize);
    const d = summaryOptions(options);
    const raw = d ? addon.summarizeGather(this._plan(), c.samples, c.starts, c.frameOffsets, names, d)
      : addon.summarizeGather(this._plan(), c.samples, c.starts, c.frameOffsets, names);
    return summaryResult(names, raw, c.frameOffsets);
  }

  getSignalSummariesAsync(features, signals, hopSize, options) {
    const names = this._checkNames(checkSummaryNames(features));
    const c = this._concatSignals(signals, hopSize);
    const d = summaryOptions(options);
    return this._runAsync((plan) => (d ? addon.summarizeGatherAsync(plan, c.samples, c.starts, c.frameOffsets, names, d)
      : addon.summarizeGatherAsync(plan, c.samples, c.starts, c.frameOffsets, names)))
      .then((r) => summaryResult(names, r, c.frameOffsets));
  }

  // The onsets of getBatchSignals' signals: the spectral flux of `feature` (one of getSignalSummaries' flux fields;
  // mode and lag as there) is the onset envelope, and its peaks are picked on the device within each signal
  // (include/meyda_gpu.h): buffer t is a candidate when no buffer of [t - preMax, t + postMax] is above it and it is
  // at least delta above the mean of [t - preAvg, t + postAvg] (each reach 0..64, the signal's first and last
  // buffers repeated beyond its ends), and the candidates are thinned so that two onsets are more than `wait`
  // buffers apart. Returns {frameOffsets, onsetOffsets, onsets}: signal s's onsets are
  // onsets[onsetOffsets[s] .. onsetOffsets[s + 1]), row numbers of the whole corpus (rows as in frameOffsets),
  // ascending; with envelope: true also `envelope`, the flux per buffer (a Float32Array). Only the onsets (and the
  // envelope when asked) cross back from the device.
  getSignalOnsets(signals, hopSize, options) {
    const o = onsetOptions(options);
    const c = this._concatSignals(signals, hopSize);
    return onsetResult(addon.onsetsGather(this._plan(), c.samples, c.starts, c.frameOffsets, o), c.frameOffsets);
  }

  getSignalOnsetsAsync(signals, hopSize, options) {
    const o = onsetOptions(options);
    const c = this._concatSignals(signals, hopSize);
    return this._runAsync((plan) => addon.onsetsGatherAsync(plan, c.samples, c.starts, c.frameOffsets, o))
      .then((r) => onsetResult(r, c.frameOffsets));
  }

  // The tempo of getBatchSignals' signals (librosa.feature.tempogram and librosa.feature.tempo on the device): the
  // spectral flux of options.feature (default 'melBands'; mode and lag as in getSignalOnsets) at options.hopSize is the
  // onset envelope; every buffer's row of the tempogram is the autocorrelation of the winLength (384) envelope values
  // around it under a window (options.window, a Float32Array of winLength, or Meyda.tempogramWindow) at the lags
  // 0 .. numLags - 1 (numLags defaults to winLength), divided by lag 0 (norm 'lag0'; 'none': the sums) in the fixed
  // order of include/meyda_gpu.h; the rows are pooled per signal and the lag is the one whose score
  // (1 + gain mean(lag)) prior(lag) is largest (gain 1e6; options.prior, a Float64Array of numLags, or
  // Meyda.tempoPrior of the frame rate sampleRate / hopSize with startBpm 120, stdOctaves 1, maxBpm 320). Returns
  // {frameOffsets, lag, bpm, numLags}: lag a Uint32Array and bpm a Float64Array of signals.length, bpm = 60 frameRate /
  // lag, NaN where the lag is 0 (no tempo: a signal without buffers); with mean: true also `mean`, the mean tempogram
  // row of every signal (a Float64Array of signals.length x numLags), with envelope: true the flux per buffer. Only
  // these cross back from the device.
  getSignalTempo(signals, options) {
    const o = tempoOptions(options, this.sampleRate);
    const c = this._concatSignals(signals, o.hopSize);
    return tempoResult(addon.tempoGather(this._plan(), c.samples, c.starts, c.frameOffsets, o.addon), c.frameOffsets, o);
  }

  getSignalTempoAsync(signals, options) {
    const o = tempoOptions(options, this.sampleRate);
    const c = this._concatSignals(signals, o.hopSize);
    return this._runAsync((plan) => addon.tempoGatherAsync(plan, c.samples, c.starts, c.frameOffsets, o.addon))
      .then((r) => tempoResult(r, c.frameOffsets, o));
  }

  // The beats of getBatchSignals' signals (librosa.beat.beat_track's tracker on the device): getSignalTempo's route gives
  // every signal's lag, which is its beat period in buffers, and the tracker of include/meyda_gpu.h places the beats on
  // the same onset envelope: a local score (the normalised envelope under a Gaussian of the period), a cumulative score
  // with the penalty tightness (100) x log^2 on the distance to the beat before, the last beat at a late local maximum,
  // the chain of back links and, with trim (true), the weak ends cut. The options are getSignalTempo's without `mean`,
  // and tightness, trim, maxPeriod (default numLags - 1, the largest lag there can be; at most 1023) or tables, a
  // Meyda.beatTables result for maxPeriod. Returns {frameOffsets, lag, bpm, numLags, beatOffsets, beats, signals}: beats
  // the buffer indices over all signals, ascending, signal s owning beats[beatOffsets[s] .. beatOffsets[s + 1]), and
  // signals[s] = {lag, bpm, beats}: the beats of signal s counted from its own first buffer.
  getSignalBeats(signals, options) {
    const o = beatOptions(options, this.sampleRate);
    const c = this._concatSignals(signals, o.hopSize);
    return beatResult(addon.beatsGather(this._plan(), c.samples, c.starts, c.frameOffsets, o.addon), c.frameOffsets, o);
  }

  getSignalBeatsAsync(signals, options) {
    const o = beatOptions(options, this.sampleRate);
    const c = this._concatSignals(signals, o.hopSize);
    return this._runAsync((plan) => addon.beatsGatherAsync(plan, c.samples, c.starts, c.frameOffsets, o.addon))
      .then((r) => beatResult(r, c.frameOffsets, o));
  }

  // The tracker's tables for the periods 1 .. maxPeriod: {gauss: Float32Array, penalty: Float64Array}. Host only.
  static beatTables(maxPeriod, tightness) {
    if (!Number.isInteger(maxPeriod) || maxPeriod < 1 || maxPeriod > 1023) throw new RangeError('maxPeriod must be an integer from 1 to 1023');
    if (tightness === undefined) tightness = 100;
    if (typeof tightness !== 'number' || !Number.isFinite(tightness) || !(tightness > 0)) {
      throw new RangeError('tightness must be a positive finite number');
    }
    return addon.beatTables(maxPeriod, tightness);
  }

  // The periodic Hann window of the tempogram, 0.5 - 0.5 cos(2 pi j / winLength): a Float32Array. Host only.
  static tempogramWindow(winLength) {
    if (!Number.isInteger(winLength) || winLength < 2 || winLength > 1024) throw new RangeError('winLength must be an integer from 2 to 1024');
    return addon.tempogramWindow(winLength);
  }

  // librosa's log-normal tempo prior over the lags 0 .. numLags - 1 of an envelope of frameRate rows a second, without
  // its constant factor: 0 at lag 0 and above maxBpm (0: no limit); options {startBpm: 120, stdOctaves: 1, maxBpm: 320}.
  // A Float64Array. Host only.
  static tempoPrior(frameRate, numLags, options) {
    if (typeof frameRate !== 'number' || !(frameRate > 0) || !Number.isFinite(frameRate)) {
      throw new RangeError('frameRate must be a positive finite number');
    }
    if (!Number.isInteger(numLags) || numLags < 1 || numLags > 1024) throw new RangeError('numLags must be an integer from 1 to 1024');
    return addon.tempoPrior(frameRate, numLags, tempoPriorOptions(options));
  }

  // The chroma of getBatchSignals' signals (later Meyda's `chroma`): every buffer's amplitude spectrum times a
  // numChroma x bufferSize / 2 filter bank, each product sum added in the fixed order of include/meyda_gpu.h, then
  // divided by the buffer's largest value (norm 'max', Meyda's; 'none': the sums). The bank is options.weights (a
  // Float32Array, numChroma rows: the caller's own, which may be signed) or Meyda.chromaFilterBank of this
  // instance's bufferSize and sample rate with {numChroma, a440, centerOctave, octaveWidth, baseC}. Returns {chroma,
  // numChroma, frameOffsets}: chroma is a Float32Array, buffer t's profile at [t numChroma, (t + 1) numChroma), rows
  // as in frameOffsets; with summary: true also `summaries`: {mean, variance, min, max}, Float64Arrays of
  // signals.length x numChroma as getSignalSummaries gives them. Only the profiles and the summaries cross back.
  getSignalChroma(signals, hopSize, options) {
    const o = chromaOptions(options, this.bufferSize, this.sampleRate);
    const c = this._concatSignals(signals, hopSize);
    return chromaResult(addon.chromaGather(this._plan(), c.samples, c.starts, c.frameOffsets, o), c.frameOffsets);
  }

  getSignalChromaAsync(signals, hopSize, options) {
    const o = chromaOptions(options, this.bufferSize, this.sampleRate);
    const c = this._concatSignals(signals, hopSize);
    return this._runAsync((plan) => addon.chromaGatherAsync(plan, c.samples, c.starts, c.frameOffsets, o))
      .then((r) => chromaResult(r, c.frameOffsets));
  }

  // The harmonic / percussive separation of getBatchSignals' signals by median filtering (Fitzgerald;
  // librosa.decompose.hpss) as include/meyda_gpu.h states it: per signal, the median of every bin over kernelTime
  // buffers and the median of every buffer over kernelFreq bins (odd, 1 to 31; kernelSize: one number for both or
  // [kernelTime, kernelFreq]; 31), the masks of power 1, 2 (the default) or Infinity (the hard mask) under margin (one
  // number or [marginHarmonic, marginPercussive], each >= 1; 1). What is asked of the parts: chroma: getSignalChroma's
  // options, for the chroma of the harmonic part (chroma, numChroma, with summary: true chromaSummaries); flux: {mode:
  // 'rectified', lag: 1, summary: false}, for the flux of the percussive part (flux, a Float32Array of one value per
  // buffer: the onset envelope; with summary fluxSummaries); harmonic: true, percussive: true for the parts themselves,
  // Float32Arrays of bufferSize / 2 values per buffer. Only what is asked for crosses back.
  getSignalHpss(signals, hopSize, options) {
    const o = hpssOptions(options, this.bufferSize, this.sampleRate);
    const c = this._concatSignals(signals, hopSize);
    return hpssResult(addon.hpssGather(this._plan(), c.samples, c.starts, c.frameOffsets, o), c.frameOffsets);
  }

  getSignalHpssAsync(signals, hopSize, options) {
    const o = hpssOptions(options, this.bufferSize, this.sampleRate);
    const c = this._concatSignals(signals, hopSize);
    return this._runAsync((plan) => addon.hpssGatherAsync(plan, c.samples, c.starts, c.frameOffsets, o))
      .then((r) => hpssResult(r, c.frameOffsets));
  }

  // The chroma filter bank of librosa.filters.chroma (later Meyda's createChromaFilterBank) as include/meyda_gpu.h
  // states it: a Float32Array of numChroma x bufferSize / 2, row-major; options {numChroma: 12, a440: 440,
  // centerOctave: 5, octaveWidth: 2 (0: no octave weighting), baseC: true (row 0 is C; false: A)}. Host only.
  static chromaFilterBank(bufferSize, sampleRate, options) {
    if (typeof bufferSize !== 'number' || !isPowerOfTwo(bufferSize) || bufferSize < 4) {
      throw new Error('Buffer size is not a power of two: Meyda will not run.');
    }
    if (typeof sampleRate !== 'number' || !(sampleRate > 0) || !Number.isFinite(sampleRate)) {
      throw new RangeError('sampleRate must be a positive finite number');
    }
    return addon.chromaWeights(bufferSize, sampleRate, chromaBankOptions(options));
  }

  _concatSignals(signals, hopSize) {
    const hop = this._checkHop(hopSize);
    if (!Array.isArray(signals)) throw new TypeError('signals must be an array of Float32Arrays');
    const xs = signals.map(toF32);
    const t = Meyda.signalsFrameStarts(xs.map((x) => x.length), this.bufferSize, hop);
    const samples = new Float32Array(xs.reduce((a, x) => a + x.length, 0));
    let at = 0;
    for (const x of xs) {
      samples.set(x, at);
      at += x.length;
    }
    return { samples, starts: t.starts, frameOffsets: t.frameOffsets };
  }

  // starts as the addon takes them (a Float64Array), checked before it is called; the device groups of
  // options.devices take dense buffers only (include/meyda_gpu.h).
  _checkStarts(starts) {
    if (Array.isArray(this.options.devices)) {
      throw new Error('starts are not supported with options.devices: device groups take dense buffers only');
    }
    return safeIntegers(starts, 'starts');
  }

  // hopSize: a positive integer (that fits the C ABI's uint32), checked before the addon is called; the
  // device groups of options.devices take dense buffers only (include/meyda_gpu.h).
  _checkHop(hopSize) {
    if (typeof hopSize !== 'number' || !Number.isInteger(hopSize) || hopSize < 1 || hopSize > 4294967295) {
      throw new RangeError('hopSize must be a positive integer, got ' + String(hopSize));
    }
    if (Array.isArray(this.options.devices)) {
      throw new Error('hopSize is not supported with options.devices: device groups take dense buffers only');
    }
    return hopSize;
  }

  // 'melBands' is an auxiliary output of the C ABI (mgx_aux_outputs), which the device groups of
  // options.devices do not take (include/meyda_gpu.h): refused here, before the addon is called.
  _checkNames(names) {
    if (Array.isArray(this.options.devices) && names.indexOf('melBands') >= 0) {
      throw new Error('melBands is not supported with options.devices: device groups take no auxiliary outputs');
    }
    return names;
  }

  static signalFrames(numSamples, bufferSize, hopSize) {
    if (typeof hopSize !== 'number' || !Number.isInteger(hopSize) || hopSize < 1 || hopSize > 4294967295) {
      throw new RangeError('hopSize must be a positive integer, got ' + String(hopSize));
    }
    return addon.signalFrames(numSamples, bufferSize, hopSize);
  }

  // The buffers of signals of the given lengths stored one after another: {starts, frameOffsets}, Float64Arrays
  // -- the start of every buffer in signal order (getBatchGather's starts), and the lengths.length + 1 prefix
  // sums of the signals' buffer counts. Host only.
  static signalsFrameStarts(lengths, bufferSize, hopSize) {
    if (typeof hopSize !== 'number' || !Number.isInteger(hopSize) || hopSize < 1 || hopSize > 4294967295) {
      throw new RangeError('hopSize must be a positive integer, got ' + String(hopSize));
    }
    if (typeof bufferSize !== 'number' || !Number.isInteger(bufferSize) || bufferSize < 1 || bufferSize > 4294967295) {
      throw new RangeError('bufferSize must be a positive integer, got ' + String(bufferSize));
    }
    return addon.signalsFrameStarts(safeIntegers(lengths, 'lengths'), bufferSize, hopSize);
  }

  static readWav(wavBytes) {
    return addon.wavParse(wavBytes);
  }

  // Per-frame view of a batch result, in the shapes get() returns.
  static frame(result, name, index, bufferSize, numMfccCoeffs, numMelBands) {
    return frameValue(name, result, index, bufferSize, numMfccCoeffs, numMelBands);
  }

  // Frees the device plans now. A plan an async job still owns is left to that job: the
  // addon keeps it alive until the job settles and the GC then frees it.
  dispose() {
    const all = Object.values(this._plans);
    // (a pooled plan with jobs still queued on it is left to them, like a busy one)
    for (const pool of Object.values(this._asyncPlans)) all.push(...pool.filter((sl) => sl.pending === 0).map((sl) => sl.plan));
    for (const p of all) if (!addon.planBusy(p)) addon.destroyPlan(p);
    this._plans = {};
    this._asyncPlans = {};
  }
}

// The output fields of the C ABI in mgx_outputs order, then mgx_aux_outputs' (the addon's extractInto
// offsets) and the result keys each requested feature fills.
const FIELDS = ['rms', 'energy', 'zcr', 'spectralCentroid', 'spectralFlatness', 'spectralSlope', 'spectralRolloff',
  'spectralSpread', 'spectralSkewness', 'spectralKurtosis', 'loudness.total', 'perceptualSpread', 'perceptualSharpness',
  'loudness.specific', 'mfcc', 'amplitudeSpectrum', 'powerSpectrum', 'complexSpectrum.real', 'complexSpectrum.imag',
  'melBands'];
const KEYS_OF = { loudness: ['loudness.specific', 'loudness.total'],
  complexSpectrum: ['complexSpectrum.real', 'complexSpectrum.imag'] };

// Output-field bits of each feature name (its FIELDS entries).
const FIELD_BITS = {};
FIELDS.forEach((k, i) => { FIELD_BITS[k] = 2 ** i; });
FIELD_BITS.loudness = FIELD_BITS['loudness.specific'] + FIELD_BITS['loudness.total'];
FIELD_BITS.complexSpectrum = FIELD_BITS['complexSpectrum.real'] + FIELD_BITS['complexSpectrum.imag'];

// Extraction of F frames into one ArrayBuffer (addon.extractInto), its layout worked out once per
// (output fields, F) and kept in the instance's `cache`: a result object of typed-array views with
// extract()'s keys and shapes (scalars as Float64Array: the facade's plans use scalarF64). One
// allocation and a few N-API calls per launch instead of an ArrayBuffer, a reference and a typed array
// per output (the real-time paths).
function extractViews(cache, plan, frames, names, N, nc, nm, scratch) {
  const F = frames.length / N;
  let bits = 0;
  for (let j = 0; j < names.length; j++) bits += FIELD_BITS[names[j]] || 0;  // (names are distinct)
  const key = F < 4194304 ? bits * 4194304 + F : bits + ':' + F;
  let lay = cache.get(key);
  if (!lay) {
    const per = (i) => (i < 13 ? 1 : i === 13 ? 24 : i === 14 ? nc : i === 19 ? nm || 26 : i < 17 ? N / 2 : N);
    // (19 offsets, the mgx_outputs fields, unless melBands is asked for: then its offset is the 20th)
    const offsets = new Float64Array(bits >= 2 ** 19 ? 20 : 19).fill(-1);
    const views = [];
    let at = 0;
    FIELDS.forEach((k, i) => {
      if (!(Math.floor(bits / 2 ** i) % 2)) return;
      const len = F * per(i), bytes = len * (i < 13 ? 8 : 4);
      offsets[i] = at;
      views.push([k, i < 13 ? Float64Array : Float32Array, at, len]);
      at += Math.ceil(bytes / 8) * 8;
    });
    lay = { offsets, views, bytes: Math.max(at, 8) };
    if (cache.size > 256) cache.clear();
    cache.set(key, lay);
  }
  // scratch: the layout's own buffer and views, reused call after call (get(): the values are copied out at
  // once); otherwise a fresh buffer whose views the caller may keep (the batched callbacks)
  if (scratch && lay.scratch) {
    addon.extractInto(plan, frames, lay.offsets, lay.scratch.ab);
    return lay.scratch.r;
  }
  const ab = new ArrayBuffer(lay.bytes);
  addon.extractInto(plan, frames, lay.offsets, ab);
  const r = {};
  const v = lay.views;
  for (let j = 0; j < v.length; j++) r[v[j][0]] = new v[j][1](ab, v[j][2], v[j][3]);
  if (scratch) lay.scratch = { ab, r };
  return r;
}

// A batched callback's value for frame i, compiled once per feature list: an object literal (or, for a
// single name, the bare value) whose entries read the batch's result arrays -- numbers, and subarray
// views where get() returns arrays -- so a callback costs an allocation, not a dispatch per feature.
const BUILDERS = new Map();
function frameBuilder(names, single) {
  const key = single !== null ? '=' + single : names.join('\u0000');
  let f = BUILDERS.get(key);
  if (f) return f;
  const expr = (n) => {
    switch (n) {
      case 'buffer': return 'x.slice(i * N, i * N + N)';
      case 'loudness': return "{ specific: r['loudness.specific'].subarray(i * 24, i * 24 + 24), total: r['loudness.total'][i] }";
      case 'mfcc': return 'r.mfcc.subarray(i * nc, i * nc + nc)';
      case 'melBands': return 'r.melBands.subarray(i * nm, i * nm + nm)';
      case 'amplitudeSpectrum': case 'powerSpectrum': return 'r.' + n + '.subarray(i * (N >> 1), i * (N >> 1) + (N >> 1))';
      case 'complexSpectrum': return "{ real: r['complexSpectrum.real'].subarray(i * N, i * N + N), " +
        "imag: r['complexSpectrum.imag'].subarray(i * N, i * N + N), length: N }";
      default: return 'r[' + JSON.stringify(n) + '][i]';
    }
  };
  const body = single !== null ? expr(single)
    : '{ ' + names.map((n) => JSON.stringify(n) + ': ' + expr(n)).join(', ') + ' }';
  f = new Function('r', 'x', 'i', 'N', 'nc', 'nm', 'return (' + body + ');');  // eslint-disable-line no-new-func
  BUILDERS.set(key, f);
  return f;
}

function toF32(frames) {
  return frames instanceof Float32Array ? frames : Float32Array.from(frames);
}

// Sample indices or lengths as the addon takes them, a Float64Array: every entry a non-negative safe integer
// (anything else -- a fraction, a negative, NaN, a non-number -- is a RangeError naming the entry).
function safeIntegers(values, what) {
  if (!Array.isArray(values) && !ArrayBuffer.isView(values)) {
    throw new TypeError(what + ' must be an array or a typed array of integers');
  }
  const out = new Float64Array(values.length);
  for (let i = 0; i < values.length; ++i) {
    const v = typeof values[i] === 'bigint' ? Number(values[i]) : values[i];
    if (typeof v !== 'number' || !Number.isSafeInteger(v) || v < 0) {
      throw new RangeError(what + '[' + i + '] must be a non-negative safe integer, got ' + String(values[i]));
    }
    out[i] = v;
  }
  return out;
}

function checkBatchNames(features) {
  const names = typeof features === 'string' ? [features] : Array.prototype.slice.call(features);
  for (const n of names) {
    if (!GPU_FEATURES.has(n)) throw new TypeError("unknown batch feature '" + n + "'");
  }
  return names;
}

// The features a summary pools: every batch feature but the complex spectrum and the buffer itself
function checkSummaryNames(features) {
  const names = typeof features === 'string' ? [features] : Array.prototype.slice.call(features);
  for (const n of names) {
    if (n === 'complexSpectrum' || n === 'buffer') throw new TypeError("'" + n + "' has no summary");
  }
  return checkBatchNames(names);
}

// The addon's summaries (per field a Float64Array, signal s's statistic k at [(4 s + k) width, ...)) in the
// facade's shape: per feature {mean, variance, min, max}, each signals x width
const STATS = ['mean', 'variance', 'min', 'max'];
function summaryResult(names, raw, frameOffsets) {
  const S = frameOffsets.length - 1;
  const split = (a) => {
    const w = S > 0 ? a.length / (STATS.length * S) : 0;
    const o = {};
    STATS.forEach((k, j) => {
      o[k] = new Float64Array(S * w);
      for (let s = 0; s < S; ++s) o[k].set(a.subarray((s * STATS.length + j) * w, (s * STATS.length + j + 1) * w), s * w);
    });
    return o;
  };
  const r = { frameOffsets };
  for (const n of names) {
    r[n] = n === 'loudness' ? { specific: split(raw['loudness.specific']), total: split(raw['loudness.total']) } : split(raw[n]);
  }
  // (the delta summaries the addon hangs on its result: the same fields, the same shape)
  for (const k of ['delta', 'delta2']) if (raw[k]) r[k] = summaryResult(names, raw[k], frameOffsets);
  // (the flux: per request the four statistics of the signals, and the per-frame column where it was asked for)
  if (raw.flux) {
    r.flux = raw.flux.map((f) => {
      const o = {};
      STATS.forEach((k, j) => {
        o[k] = new Float64Array(S);
        for (let s = 0; s < S; ++s) o[k][s] = f.summary[s * STATS.length + j];
      });
      if (f.perFrame) o.perFrame = f.perFrame;
      return o;
    });
  }
  return r;
}

// The fields a flux is taken of and its modes, as mgx_flux_request numbers them
const FLUX_FIELDS = { loudness: 13, mfcc: 14, amplitudeSpectrum: 15, powerSpectrum: 16, melBands: 19 };
const FLUX_MODES = { rectified: 0, l1: 1, l2: 2 };

// getSignalSummaries' options as the addon takes them (the delta options, and flux in the library's numbers), or
// null when neither deltas nor flux are asked for
function summaryOptions(options) {
  const d = deltaOptions(options);
  if (options === undefined || options === null || options.flux === undefined) return d;
  if (!Array.isArray(options.flux) || options.flux.length < 1 || options.flux.length > 4) {
    throw new RangeError('flux must be an array of 1 to 4 requests');
  }
  const flux = options.flux.map((f) => {
    if (f === null || typeof f !== 'object') throw new TypeError('a flux request must be an object: {feature, mode, lag, perFrame}');
    if (!Object.prototype.hasOwnProperty.call(FLUX_FIELDS, f.feature)) throw new TypeError("'" + f.feature + "' has no flux");
    const mode = f.mode === undefined ? 'rectified' : f.mode;
    if (!Object.prototype.hasOwnProperty.call(FLUX_MODES, mode)) throw new RangeError("flux mode must be 'rectified', 'l1' or 'l2'");
    const lag = f.lag === undefined ? 1 : f.lag;
    if (!Number.isInteger(lag) || lag < 1 || lag > 8) throw new RangeError('flux lag must be an integer from 1 to 8');
    return { field: FLUX_FIELDS[f.feature], mode: FLUX_MODES[mode], lag, perFrame: !!f.perFrame };
  });
  return Object.assign({}, d || {}, { flux });
}

// getSignalOnsets' options as the addon takes them (the flux in the library's numbers)
function onsetOptions(options) {
  if (options === undefined || options === null || typeof options !== 'object') {
    throw new TypeError('options must be an object: {feature, mode, lag, preMax, postMax, preAvg, postAvg, delta, wait, envelope}');
  }
  if (!Object.prototype.hasOwnProperty.call(FLUX_FIELDS, options.feature)) throw new TypeError("'" + options.feature + "' has no flux");
  const mode = options.mode === undefined ? 'rectified' : options.mode;
  if (!Object.prototype.hasOwnProperty.call(FLUX_MODES, mode)) throw new RangeError("flux mode must be 'rectified', 'l1' or 'l2'");
  const lag = options.lag === undefined ? 1 : options.lag;
  if (!Number.isInteger(lag) || lag < 1 || lag > 8) throw new RangeError('flux lag must be an integer from 1 to 8');
  const o = { field: FLUX_FIELDS[options.feature], mode: FLUX_MODES[mode], lag, envelope: !!options.envelope };
  for (const k of ['preMax', 'postMax', 'preAvg', 'postAvg']) {
    o[k] = options[k] === undefined ? 0 : options[k];
    if (!Number.isInteger(o[k]) || o[k] < 0 || o[k] > 64) throw new RangeError(k + ' must be an integer from 0 to 64');
  }
  o.wait = options.wait === undefined ? 0 : options.wait;
  if (!Number.isInteger(o.wait) || o.wait < 0 || o.wait > 4294967295) throw new RangeError('wait must be an integer from 0 to 4294967295');
  o.delta = options.delta === undefined ? 0 : options.delta;
  if (typeof o.delta !== 'number') throw new TypeError('delta must be a number');
  if (Number.isNaN(o.delta)) throw new RangeError('delta must not be NaN');
  return o;
}

// Meyda.tempoPrior's options as the addon takes them
const TEMPOGRAM_NORMS = { none: 0, lag0: 1 };
function tempoPriorOptions(options) {
  if (options === undefined || options === null) options = {};
  if (typeof options !== 'object') throw new TypeError('options must be an object: {startBpm, stdOctaves, maxBpm}');
  const o = { startBpm: options.startBpm === undefined ? 120 : options.startBpm,
    stdOctaves: options.stdOctaves === undefined ? 1 : options.stdOctaves,
    maxBpm: options.maxBpm === undefined ? 320 : options.maxBpm };
  for (const k of ['startBpm', 'stdOctaves']) {
    if (typeof o[k] !== 'number' || !Number.isFinite(o[k]) || !(o[k] > 0)) throw new RangeError(k + ' must be a positive finite number');
  }
  if (typeof o.maxBpm !== 'number' || !Number.isFinite(o.maxBpm) || o.maxBpm < 0) throw new RangeError('maxBpm must be a finite number, 0 or above');
  return o;
}

// getSignalTempo's options: the hop, the frame rate, and what the addon takes (the flux in the library's numbers, the
// window and the prior as arrays)
function tempoOptions(options, sampleRate) {
  if (options === undefined || options === null || typeof options !== 'object') {
    throw new TypeError('options must be an object: {hopSize, feature, mode, lag, winLength, numLags, norm, gain, startBpm, stdOctaves, ' +
      'maxBpm, window, prior, mean, envelope}');
  }
  const hopSize = options.hopSize;
  if (!Number.isInteger(hopSize) || hopSize < 1) throw new RangeError('hopSize must be a positive integer');
  const feature = options.feature === undefined ? 'melBands' : options.feature;
  if (!Object.prototype.hasOwnProperty.call(FLUX_FIELDS, feature)) throw new TypeError("'" + feature + "' has no flux");
  const mode = options.mode === undefined ? 'rectified' : options.mode;
  if (!Object.prototype.hasOwnProperty.call(FLUX_MODES, mode)) throw new RangeError("flux mode must be 'rectified', 'l1' or 'l2'");
  const lag = options.lag === undefined ? 1 : options.lag;
  if (!Number.isInteger(lag) || lag < 1 || lag > 8) throw new RangeError('flux lag must be an integer from 1 to 8');
  const winLength = options.winLength === undefined ? 384 : options.winLength;
  if (!Number.isInteger(winLength) || winLength < 2 || winLength > 1024) throw new RangeError('winLength must be an integer from 2 to 1024');
  const numLags = options.numLags === undefined ? winLength : options.numLags;
  if (!Number.isInteger(numLags) || numLags < 1 || numLags > winLength) throw new RangeError('numLags must be an integer from 1 to winLength');
  const norm = options.norm === undefined ? 'lag0' : options.norm;
  if (!Object.prototype.hasOwnProperty.call(TEMPOGRAM_NORMS, norm)) throw new RangeError("tempogram norm must be 'lag0' or 'none'");
  const gain = options.gain === undefined ? 1e6 : options.gain;
  if (typeof gain !== 'number' || !Number.isFinite(gain) || gain < 0) throw new RangeError('gain must be a finite number, 0 or above');
  const frameRate = sampleRate / hopSize;
  let window = options.window, prior = options.prior;
  if (window === undefined || window === null) window = addon.tempogramWindow(winLength);
  else if (!(window instanceof Float32Array) || window.length !== winLength) throw new TypeError('window must be a Float32Array of winLength values');
  if (prior === undefined || prior === null) prior = addon.tempoPrior(frameRate, numLags, tempoPriorOptions(options));
  else if (!(prior instanceof Float64Array) || prior.length !== numLags) throw new TypeError('prior must be a Float64Array of numLags values');
  return { hopSize, frameRate, mean: !!options.mean,
    addon: { field: FLUX_FIELDS[feature], mode: FLUX_MODES[mode], lag, winLength, numLags, norm: TEMPOGRAM_NORMS[norm], gain, window, prior,
      mean: !!options.mean, envelope: !!options.envelope } };
}

function tempoResult(raw, frameOffsets, o) {
  const S = frameOffsets.length - 1, L = raw.numLags;
  const r = { frameOffsets, lag: raw.lag, bpm: new Float64Array(S), numLags: L };
  for (let s = 0; s < S; ++s) r.bpm[s] = raw.lag[s] > 0 ? 60 * o.frameRate / raw.lag[s] : NaN;
  if (o.mean && raw.summary) {
    r.mean = new Float64Array(S * L);
    for (let s = 0; s < S; ++s) r.mean.set(raw.summary.subarray(s * STATS.length * L, (s * STATS.length + 1) * L), s * L);
  }
  if (raw.envelope) r.envelope = raw.envelope;
  return r;
}

// getSignalBeats' options: getSignalTempo's, and the tracker's as the addon takes them (the tables as arrays)
function beatOptions(options, sampleRate) {
  const o = tempoOptions(options, sampleRate);
  if (options.mean) throw new TypeError('getSignalBeats has no mean: getSignalTempo returns the mean tempogram rows');
  const reach = Math.max(o.addon.numLags - 1, 1);
  const maxPeriod = options.maxPeriod === undefined ? reach : options.maxPeriod;
  if (!Number.isInteger(maxPeriod) || maxPeriod < reach || maxPeriod > 1023) {
    throw new RangeError('maxPeriod must be an integer from numLags - 1 to 1023');
  }
  const tightness = options.tightness === undefined ? 100 : options.tightness;
  if (typeof tightness !== 'number' || !Number.isFinite(tightness) || !(tightness > 0)) {
    throw new RangeError('tightness must be a positive finite number');
  }
  let tables = options.tables;
  if (tables === undefined || tables === null) tables = addon.beatTables(maxPeriod, tightness);
  else if (typeof tables !== 'object' || !(tables.gauss instanceof Float32Array) || !(tables.penalty instanceof Float64Array) ||
    tables.gauss.length !== (maxPeriod + 1) * (maxPeriod + 2) / 2 || tables.penalty.length !== (maxPeriod + 1) * (maxPeriod + 1)) {
    throw new TypeError('tables must be a Meyda.beatTables result for maxPeriod');
  }
  delete o.addon.mean;
  Object.assign(o.addon, { maxPeriod, trim: options.trim === undefined ? true : !!options.trim, gauss: tables.gauss, penalty: tables.penalty });
  return o;
}

function beatResult(raw, frameOffsets, o) {
  const r = tempoResult(raw, frameOffsets, o);
  r.beatOffsets = raw.beatOffsets;
  r.beats = raw.beats;
  r.signals = [];
  for (let s = 0; s + 1 < frameOffsets.length; ++s) {
    const rows = raw.beats.slice(raw.beatOffsets[s], raw.beatOffsets[s + 1]);
    for (let i = 0; i < rows.length; ++i) rows[i] -= frameOffsets[s];
    r.signals.push({ lag: r.lag[s], bpm: r.bpm[s], beats: rows });
  }
  return r;
}

// Meyda.chromaFilterBank's options as the addon takes them
const CHROMA_NORMS = { none: 0, max: 1 };
function chromaBankOptions(options) {
  if (options === undefined || options === null) options = {};
  if (typeof options !== 'object') throw new TypeError('options must be an object: {numChroma, a440, centerOctave, octaveWidth, baseC}');
  const o = { numChroma: options.numChroma === undefined ? 12 : options.numChroma,
    a440: options.a440 === undefined ? 440 : options.a440,
    centerOctave: options.centerOctave === undefined ? 5 : options.centerOctave,
    octaveWidth: options.octaveWidth === undefined ? 2 : options.octaveWidth,
    baseC: options.baseC === undefined ? true : !!options.baseC };
  if (!Number.isInteger(o.numChroma) || o.numChroma < 1 || o.numChroma > 36) throw new RangeError('numChroma must be an integer from 1 to 36');
  if (typeof o.a440 !== 'number' || !Number.isFinite(o.a440) || !(o.a440 > 0)) throw new RangeError('a440 must be a positive finite number');
  if (typeof o.centerOctave !== 'number' || !Number.isFinite(o.centerOctave)) throw new RangeError('centerOctave must be a finite number');
  if (typeof o.octaveWidth !== 'number' || !Number.isFinite(o.octaveWidth) || o.octaveWidth < 0) {
    throw new RangeError('octaveWidth must be a finite number, 0 or above');
  }
  return o;
}

// getSignalChroma's options as the addon takes them: the bank (the caller's, or the library's), its rows, the norm
function chromaOptions(options, bufferSize, sampleRate) {
  if (options === undefined || options === null) options = {};
  if (typeof options !== 'object') {
    throw new TypeError('options must be an object: {weights, numChroma, a440, centerOctave, octaveWidth, baseC, norm, summary}');
  }
  const norm = options.norm === undefined ? 'max' : options.norm;
  if (!Object.prototype.hasOwnProperty.call(CHROMA_NORMS, norm)) throw new RangeError("chroma norm must be 'max' or 'none'");
  const o = { norm: CHROMA_NORMS[norm], summary: !!options.summary };
  if (options.weights !== undefined && options.weights !== null) {
    if (!(options.weights instanceof Float32Array)) throw new TypeError('weights must be a Float32Array');
    const cols = bufferSize / 2;
    o.numChroma = options.numChroma === undefined ? options.weights.length / cols : options.numChroma;
    if (!Number.isInteger(o.numChroma) || o.numChroma < 1 || o.numChroma > 36 || o.numChroma * cols !== options.weights.length) {
      throw new RangeError('weights must hold numChroma (1 to 36) rows of bufferSize / 2 values');
    }
    o.weights = options.weights;
  } else {
    const b = chromaBankOptions(options);
    o.numChroma = b.numChroma;
    o.weights = addon.chromaWeights(bufferSize, sampleRate, b);
  }
  return o;
}

function chromaResult(raw, frameOffsets) {
  const r = { chroma: raw.chroma, numChroma: raw.numChroma, frameOffsets };
  if (raw.summary) {
    const S = frameOffsets.length - 1, w = raw.numChroma;
    r.summaries = {};
    STATS.forEach((k, j) => {
      r.summaries[k] = new Float64Array(S * w);
      for (let s = 0; s < S; ++s) r.summaries[k].set(raw.summary.subarray((s * STATS.length + j) * w, (s * STATS.length + j + 1) * w), s * w);
    });
  }
  return r;
}

// getSignalHpss' options as the addon takes them
const HPSS_MODES = { 1: 1, 2: 2, Infinity: 3 };  // power -> mgx_hpss_mode (0: the medians themselves)
function pairOf(v, dflt, what) {
  if (v === undefined || v === null) return [dflt, dflt];
  if (Array.isArray(v)) {
    if (v.length !== 2) throw new TypeError(what + ' must be one number or a pair');
    return [v[0], v[1]];
  }
  return [v, v];
}
function hpssOptions(options, bufferSize, sampleRate) {
  if (options === undefined || options === null || typeof options !== 'object') {
    throw new TypeError('options must be an object: {kernelSize, power, margin, chroma, flux, harmonic, percussive}');
  }
  const [kernelTime, kernelFreq] = pairOf(options.kernelSize, 31, 'kernelSize');
  for (const k of [kernelTime, kernelFreq]) {
    if (!Number.isInteger(k) || k < 1 || k > 31 || k % 2 !== 1) throw new RangeError('kernelSize must be odd integers from 1 to 31');
  }
  const power = options.power === undefined ? 2 : options.power;
  if (typeof power !== 'number') throw new TypeError('power must be 1, 2 or Infinity');
  if (!Object.prototype.hasOwnProperty.call(HPSS_MODES, power)) throw new RangeError('power must be 1, 2 or Infinity');
  const [marginHarmonic, marginPercussive] = pairOf(options.margin, 1, 'margin');
  for (const m of [marginHarmonic, marginPercussive]) {
    if (typeof m !== 'number') throw new TypeError('margin must be numbers');
    if (!Number.isFinite(m) || !(m >= 1)) throw new RangeError('margin must be finite numbers, 1 or above');
  }
  const o = { kernelTime, kernelFreq, mode: HPSS_MODES[power], marginHarmonic, marginPercussive,
    harmonic: !!options.harmonic, percussive: !!options.percussive };
  if (options.chroma !== undefined && options.chroma !== null && options.chroma !== false) {
    const c = chromaOptions(options.chroma === true ? {} : options.chroma, bufferSize, sampleRate);
    o.chroma = { weights: c.weights, numChroma: c.numChroma, norm: c.norm, perFrame: true, summary: c.summary };
  }
  if (options.flux !== undefined && options.flux !== null && options.flux !== false) {
    const f = options.flux === true ? {} : options.flux;
    if (typeof f !== 'object') throw new TypeError('flux must be an object: {mode, lag, summary}');
    const mode = f.mode === undefined ? 'rectified' : f.mode;
    if (!Object.prototype.hasOwnProperty.call(FLUX_MODES, mode)) throw new RangeError("flux mode must be 'rectified', 'l1' or 'l2'");
    const lag = f.lag === undefined ? 1 : f.lag;
    if (!Number.isInteger(lag) || lag < 1 || lag > 8) throw new RangeError('flux lag must be an integer from 1 to 8');
    o.flux = { mode: FLUX_MODES[mode], lag, perFrame: true, summary: !!f.summary };
  }
  if (!o.harmonic && !o.percussive && !o.chroma && !o.flux) {
    throw new TypeError('nothing asked for: one of chroma, flux, harmonic, percussive');
  }
  return o;
}

function hpssResult(raw, frameOffsets) {
  const S = frameOffsets.length - 1;
  const r = { frameOffsets };
  const stats = (flat, w) => {
    const out = {};
    STATS.forEach((k, j) => {
      out[k] = new Float64Array(S * w);
      for (let s = 0; s < S; ++s) out[k].set(flat.subarray((s * STATS.length + j) * w, (s * STATS.length + j + 1) * w), s * w);
    });
    return out;
  };
  if (raw.harmonic) r.harmonic = raw.harmonic;
  if (raw.percussive) r.percussive = raw.percussive;
  if (raw.chroma) {
    r.chroma = raw.chroma;
    r.numChroma = raw.numChroma;
  }
  if (raw.chromaSummary) r.chromaSummaries = stats(raw.chromaSummary, raw.numChroma);
  if (raw.flux) r.flux = raw.flux;
  if (raw.fluxSummary) r.fluxSummaries = stats(raw.fluxSummary, 1);
  return r;
}

function onsetResult(raw, frameOffsets) {
  const r = { frameOffsets, onsetOffsets: raw.onsetOffsets, onsets: raw.onsets };
  if (raw.envelope) r.envelope = raw.envelope;
  return r;
}

// getSignalSummaries' options as the addon takes them, or null when no deltas are asked for
function deltaOptions(options) {
  if (options === undefined || options === null) return null;
  if (typeof options !== 'object') throw new TypeError('options must be an object: {deltaWidth, deltaOrder}');
  if (options.deltaWidth === undefined && options.deltaOrder === undefined) return null;
  const d = { deltaWidth: options.deltaWidth === undefined ? 2 : options.deltaWidth,
    deltaOrder: options.deltaOrder === undefined ? 2 : options.deltaOrder };
  if (!Number.isInteger(d.deltaWidth) || d.deltaWidth < 1 || d.deltaWidth > 8) throw new RangeError('deltaWidth must be an integer from 1 to 8');
  if (d.deltaOrder !== 1 && d.deltaOrder !== 2) throw new RangeError('deltaOrder must be 1 or 2');
  return d;
}

// Slice frame `i` of a SoA batch result into the reference's return shapes
// (src/feature-info.js): numbers, Float32Array, {specific, total}, {real, imag}.
function frameValue(name, r, i, n, ncoef, nmel) {
  ncoef = ncoef || 13;
  nmel = nmel || 26;
  const L = n / 2;
  switch (name) {
    case 'loudness':
      return { specific: r['loudness.specific'].slice(i * 24, i * 24 + 24), total: r['loudness.total'][i] };
    case 'mfcc':
      return r.mfcc.slice(i * ncoef, i * ncoef + ncoef);
    case 'melBands':
      return r.melBands.slice(i * nmel, i * nmel + nmel);
    case 'amplitudeSpectrum':
      return r.amplitudeSpectrum.slice(i * L, i * L + L);
    case 'powerSpectrum':
      return r.powerSpectrum.slice(i * L, i * L + L);
    case 'complexSpectrum': {
      const real = r['complexSpectrum.real'].slice(i * n, i * n + n);
      const imag = r['complexSpectrum.imag'].slice(i * n, i * n + n);
      return { real, imag, length: n };
    }
    default:
      return r[name][i];
  }
}

module.exports = Meyda;
module.exports.Meyda = Meyda;
module.exports.isPowerOfTwo = isPowerOfTwo;
module.exports.featureInfo = FEATURE_INFO;
module.exports.addon = addon;
