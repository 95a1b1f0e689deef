'use strict';
// GPU check of getSignalTempo / getSignalTempoAsync through the facade and the N-API addon: three signals (one without
// buffers); the lags and the mean tempogram rows against the Python binding's (Plan.tempo_signals, written by
// tests/test_js_tempo_gpu.py to DIR as raw files tempo.lag.u32, tempo.mean.f64, tempo.envelope.f32 and, for the
// library's defaults, tempo384.lag.u32), the bpm arithmetic, the async form against the synchronous one, a caller's
// window and prior, and the addon's own refusals. Needs an MI355X.
// usage: node tempo_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 256, H = 64, SR = 44100;
process.on('unhandledRejection', (e) => { console.error(e); process.exit(1); });

function sameBits(a, b, what) {
  assert.ok(a.constructor === b.constructor && a.length === b.length, what);
  const x = new Uint8Array(a.buffer, a.byteOffset, a.byteLength), y = new Uint8Array(b.buffer, b.byteOffset, b.byteLength);
  for (let i = 0; i < x.length; i++) assert.ok(x[i] === y[i], what + ' byte ' + i);
}

function expected(name, T) {
  const raw = fs.readFileSync(path.join(dir, name));
  return new T(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
}

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  // three signals: many buffers and a partial tail, fewer samples than one buffer, the rest
  const cuts = [0, 600 * H + N + 7, 600 * H + N + 7 + N - 1, x.length];
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: SR }, null, N, null, { numMelBands: 40 });
  // (689 rows a second: the prior is centred on the clicks' 24 rows, 1722.66 bpm, and has no upper limit)
  const PRIOR = { startBpm: 1722.65625, maxBpm: 0 };
  const opts = Object.assign({ hopSize: H, winLength: 64, numLags: 48, mean: true, envelope: true }, PRIOR);
  const r = m.getSignalTempo(signals, opts);
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags', 'mean', 'envelope']);
  const batch = m.getBatchSignals('rms', signals, H);
  sameBits(r.frameOffsets, batch.frameOffsets, 'frameOffsets');
  const F = r.frameOffsets[3];
  assert.ok(r.lag instanceof Uint32Array && r.lag.length === 3 && r.numLags === 48);
  sameBits(r.lag, expected('tempo.lag.u32', Uint32Array), 'lag');
  assert.ok(r.mean instanceof Float64Array && r.mean.length === 3 * 48);
  sameBits(r.mean, expected('tempo.mean.f64', Float64Array), 'mean');
  assert.ok(r.envelope instanceof Float32Array && r.envelope.length === F);
  sameBits(r.envelope, expected('tempo.envelope.f32', Float32Array), 'envelope');
  // the signal without buffers: no tempo; the others: lag 0 of a normalised row is exactly 1, and a tempo
  assert.ok(r.lag[1] === 0 && Number.isNaN(r.bpm[1]) && Number.isNaN(r.mean[48]));
  for (const s of [0, 2]) {
    assert.ok(r.lag[s] > 0 && r.mean[s * 48] === 1);
    assert.strictEqual(r.bpm[s], 60 * (SR / H) / r.lag[s]);
  }
  console.log('ok tempo: the shapes, the empty signal, the Python binding\'s values, the bpm');

  const ra = await m.getSignalTempoAsync(signals, opts);
  assert.deepStrictEqual(Object.keys(ra), Object.keys(r));
  for (const k of ['lag', 'bpm', 'mean', 'envelope']) sameBits(ra[k], r[k], 'async ' + k);
  console.log('ok the async form agrees');

  // the library's defaults (W = L = 384); the window and the prior handed in are the ones the call builds
  const d = m.getSignalTempo(signals, { hopSize: H });
  assert.deepStrictEqual(Object.keys(d), ['frameOffsets', 'lag', 'bpm', 'numLags']);
  assert.strictEqual(d.numLags, 384);
  sameBits(d.lag, expected('tempo384.lag.u32', Uint32Array), 'the defaults');
  const own = m.getSignalTempo(signals, { hopSize: H, winLength: 64, numLags: 48, mean: true,
    window: Meyda.tempogramWindow(64), prior: Meyda.tempoPrior(SR / H, 48, PRIOR) });
  sameBits(own.lag, r.lag, 'window and prior handed in: lag');
  sameBits(own.mean, r.mean, 'window and prior handed in: mean');
  // a prior that allows one lag alone picks it
  const one = new Float64Array(48);
  one[5] = 1;
  const forced = m.getSignalTempo(signals, { hopSize: H, winLength: 64, numLags: 48, prior: one });
  assert.deepStrictEqual(Array.from(forced.lag), [5, 0, 5]);
  console.log('ok the defaults, a window and a prior handed in');

  // the addon's own checks, past the facade's
  const st = Meyda.signalsFrameStarts(signals.map((s) => s.length), N, H);
  const w = Meyda.tempogramWindow(64), p = Meyda.tempoPrior(SR / H, 48);
  const call = (o, fo) => Meyda.addon.tempoGather(m._plan(), x, st.starts, fo === undefined ? st.frameOffsets : fo, o);
  assert.throws(() => call({ winLength: 64, numLags: 48, window: w, prior: p }), TypeError);            // no field
  assert.throws(() => call({ field: 19, winLength: 64, numLags: 48, prior: p }), TypeError);            // no window
  assert.throws(() => call({ field: 19, winLength: 64, numLags: 48, window: w }), TypeError);           // no prior
  assert.throws(() => call({ field: 19, winLength: 64, numLags: 65, window: w, prior: p }), RangeError);
  assert.throws(() => call({ field: 19, winLength: 32, numLags: 32, window: w, prior: p }), RangeError); // the window's length
  assert.throws(() => call({ field: 19, winLength: 64, numLags: 48, window: w, prior: p, gain: -1 }), RangeError);
  assert.throws(() => call({ field: 19, winLength: 64, numLags: 48, window: w, prior: p }, new Float64Array([0])), RangeError);
  assert.throws(() => call({ field: 3, winLength: 64, numLags: 48, window: w, prior: p }), Error);       // rms has no flux
  m.dispose();
  console.log('tempo_gpu: 4 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
