'use strict';
// GPU check of getSignalHpss / getSignalHpssAsync through the facade and the N-API addon: three signals (one without
// buffers); the two parts, the chroma of the harmonic part, the flux of the percussive part and their summaries
// against the Python binding's (Plan.hpss_signals, written by tests/test_js_hpss_gpu.py to DIR as raw files
// hpss.NAME.f32 / hpss.NAME.STAT.f64 and hard.NAME.f32), the async form against the synchronous one, and the addon's own
// refusals. Needs an MI355X.
// usage: node hpss_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 1024, H = 128;
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
  const cuts = [0, 9 * N + 77, 9 * N + 77 + N - 1, x.length];
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: 44100 }, null, N, null, {});
  const opts = { kernelSize: [17, 31], margin: [2, 1.5], harmonic: true, percussive: true, chroma: { summary: true },
    flux: { mode: 'rectified', lag: 2, summary: true } };
  const r = m.getSignalHpss(signals, H, opts);
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'harmonic', 'percussive', 'chroma', 'numChroma', 'chromaSummaries', 'flux', 'fluxSummaries']);
  const batch = m.getBatchSignals('rms', signals, H);
  sameBits(r.frameOffsets, batch.frameOffsets, 'frameOffsets');
  const F = r.frameOffsets[3];
  assert.ok(r.harmonic.length === F * N / 2 && r.percussive.length === F * N / 2 && r.chroma.length === F * 12 && r.flux.length === F);
  for (const k of ['harmonic', 'percussive', 'chroma', 'flux']) sameBits(r[k], expected('hpss.' + k + '.f32', Float32Array), k);
  for (const k of ['mean', 'variance', 'min', 'max']) {
    sameBits(r.chromaSummaries[k], expected('hpss.chroma.' + k + '.f64', Float64Array), 'chromaSummaries.' + k);
    sameBits(r.fluxSummaries[k], expected('hpss.flux.' + k + '.f64', Float64Array), 'fluxSummaries.' + k);
    assert.ok(Number.isNaN(r.fluxSummaries[k][1]), 'the signal without buffers is NaN');
  }
  console.log('ok hpss: the shapes, the empty signal, the Python binding\'s values');

  const ra = await m.getSignalHpssAsync(signals, H, opts);
  assert.deepStrictEqual(Object.keys(ra), Object.keys(r));
  for (const k of ['harmonic', 'percussive', 'chroma', 'flux']) sameBits(ra[k], r[k], 'async ' + k);
  for (const k of ['mean', 'variance', 'min', 'max']) sameBits(ra.chromaSummaries[k], r.chromaSummaries[k], 'async ' + k);
  console.log('ok the async form agrees');

  // the hard mask with the default kernels, one part alone
  const hard = m.getSignalHpss(signals, H, { power: Infinity, percussive: true });
  assert.deepStrictEqual(Object.keys(hard), ['frameOffsets', 'percussive']);
  sameBits(hard.percussive, expected('hard.percussive.f32', Float32Array), 'hard mask');
  console.log('ok the hard mask, one part alone');

  // the addon's own checks, past the facade's
  const st = Meyda.signalsFrameStarts(signals.map((s) => s.length), N, H);
  const call = (o, fo) => Meyda.addon.hpssGather(m._plan(), x, st.starts, fo === undefined ? st.frameOffsets : fo, o);
  assert.throws(() => call(3), TypeError);
  assert.throws(() => call({}), RangeError);  // nothing asked for
  for (const kernelTime of [0, 2, 32, 33]) assert.throws(() => call({ kernelTime, harmonic: true }), RangeError);
  assert.throws(() => call({ kernelFreq: 4, harmonic: true }), RangeError);
  assert.throws(() => call({ mode: 4, harmonic: true }), RangeError);
  for (const marginHarmonic of [0.5, Infinity, 1e39]) assert.throws(() => call({ marginHarmonic, harmonic: true }), RangeError);
  assert.throws(() => call({ chroma: { numChroma: 12 } }), TypeError);
  assert.throws(() => call({ flux: { summary: true } }, null), RangeError);
  assert.throws(() => call({ flux: { perFrame: false } }), RangeError);
  m.dispose();
  console.log('hpss_gpu: 4 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
