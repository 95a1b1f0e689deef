'use strict';
// Host-side checks of the facade's HPSS plumbing (meyda.js getSignalHpss / getSignalHpssAsync) against a stand-in
// addon that records its calls (tests/js/hpss_addon.js): what reaches the addon, the defaults, the shapes that come
// back, and that a bad option never reaches it. The GPU results themselves: tests/js/hpss_gpu.js.
const path = require('path');
const assert = require('assert');
process.env.MEYDA_AMD_ADDON = path.join(__dirname, 'hpss_addon.js');
const mock = require('./hpss_addon');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

let n = 0;
function check(name, fn) { fn(); n++; console.log('ok ' + name); }
const N = 256, H = 64, SR = 44100;
const m = new Meyda({ sampleRate: SR }, null, N);
const signals = [new Float32Array(N - 1), new Float32Array(N + 9 * H), new Float32Array(N), new Float32Array(N + 2 * H + 5)];
const gathers = () => mock.calls.filter((c) => c.fn.startsWith('hpssGather'));

check('the defaults reach the addon', () => {
  mock.calls.length = 0;
  const r = m.getSignalHpss(signals, H, { chroma: {}, flux: {} });
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['chromaWeights', 'hpssGather']);
  const [samples, starts, fo, o] = mock.calls[1].args;
  assert.strictEqual(samples.length, signals.reduce((a, x) => a + x.length, 0));
  assert.deepStrictEqual(Array.from(fo), [0, 0, 10, 11, 14]);
  assert.strictEqual(starts.length, 14);
  assert.deepStrictEqual(Object.keys(o), ['kernelTime', 'kernelFreq', 'mode', 'marginHarmonic', 'marginPercussive', 'harmonic', 'percussive',
    'chroma', 'flux']);
  assert.deepStrictEqual([o.kernelTime, o.kernelFreq, o.mode, o.marginHarmonic, o.marginPercussive, o.harmonic, o.percussive],
    [31, 31, 2, 1, 1, false, false]);
  assert.deepStrictEqual(Object.keys(o.chroma), ['weights', 'numChroma', 'norm', 'perFrame', 'summary']);
  assert.ok(o.chroma.weights instanceof Float32Array && o.chroma.weights.length === 12 * N / 2);
  assert.deepStrictEqual([o.chroma.numChroma, o.chroma.norm, o.chroma.perFrame, o.chroma.summary], [12, 1, true, false]);
  assert.deepStrictEqual(o.flux, { mode: 0, lag: 1, perFrame: true, summary: false });
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'chroma', 'numChroma', 'flux']);
  assert.ok(r.chroma.length === 14 * 12 && r.flux.length === 14 && r.numChroma === 12);
});

check('the options reach the addon in the library\'s numbers', () => {
  mock.calls.length = 0;
  const weights = new Float32Array(5 * N / 2).fill(1);
  const r = m.getSignalHpss(signals, H, { kernelSize: [5, 17], power: Infinity, margin: [2, 1.5], harmonic: true, percussive: 1,
    chroma: { weights, norm: 'none', summary: true }, flux: { mode: 'l2', lag: 3, summary: true } });
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['hpssGather']);  // the caller's bank: none is built
  const o = mock.calls[0].args[3];
  assert.deepStrictEqual([o.kernelTime, o.kernelFreq, o.mode, o.marginHarmonic, o.marginPercussive, o.harmonic, o.percussive],
    [5, 17, 3, 2, 1.5, true, true]);
  assert.ok(o.chroma.weights === weights && o.chroma.numChroma === 5 && o.chroma.norm === 0 && o.chroma.summary === true);
  assert.deepStrictEqual(o.flux, { mode: 2, lag: 3, perFrame: true, summary: true });
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'harmonic', 'percussive', 'chroma', 'numChroma', 'chromaSummaries', 'flux', 'fluxSummaries']);
  assert.ok(r.harmonic.length === 14 * 128 && r.percussive.length === 14 * 128);
  // the summaries per statistic: signals x width, from the addon's signals x 4 x width
  assert.deepStrictEqual(Object.keys(r.chromaSummaries), ['mean', 'variance', 'min', 'max']);
  assert.deepStrictEqual(Array.from(r.chromaSummaries.variance.subarray(5, 10)), [25, 26, 27, 28, 29]);
  assert.deepStrictEqual(Array.from(r.fluxSummaries.mean), [0, 4, 8, 12]);
  assert.deepStrictEqual(Array.from(r.fluxSummaries.max), [3, 7, 11, 15]);
  // one number for both kernels and both margins; the powers
  for (const [power, mode] of [[1, 1], [2, 2], [Infinity, 3]]) {
    mock.calls.length = 0;
    m.getSignalHpss(signals, H, { kernelSize: 7, margin: 3, power, harmonic: true });
    const q = mock.calls[0].args[3];
    assert.deepStrictEqual([q.kernelTime, q.kernelFreq, q.mode, q.marginHarmonic, q.marginPercussive], [7, 7, mode, 3, 3]);
    assert.ok(q.chroma === undefined && q.flux === undefined);
  }
});

check('a bad option never reaches the addon', () => {
  mock.calls.length = 0;
  const bad = (o, E) => assert.throws(() => m.getSignalHpss(signals, H, o), E);
  bad(undefined, TypeError);
  bad(3, TypeError);
  bad({}, TypeError);  // nothing asked for
  for (const kernelSize of [0, 2, 30, 32, 33, 1.5, '31', [31, 2], [4, 31], [0, 1]]) bad({ kernelSize, harmonic: true }, RangeError);
  bad({ kernelSize: [3, 5, 7], harmonic: true }, TypeError);
  for (const power of [0, 3, 1.5, -1, NaN]) bad({ power, harmonic: true }, RangeError);
  bad({ power: '2', harmonic: true }, TypeError);
  for (const margin of [0, 0.999, -2, Infinity, NaN, [1, 0.5], [0.5, 1], [Infinity, 1]]) bad({ margin, harmonic: true }, RangeError);
  bad({ margin: '1', harmonic: true }, TypeError);
  bad({ margin: [1, 2, 3], harmonic: true }, TypeError);
  bad({ chroma: { norm: 'l2' } }, RangeError);
  bad({ chroma: { numChroma: 37 } }, RangeError);
  bad({ chroma: { weights: new Float32Array(100) } }, RangeError);
  bad({ chroma: 3 }, TypeError);
  bad({ flux: { mode: 'l3' } }, RangeError);
  for (const lag of [0, 9, 1.5]) bad({ flux: { lag } }, RangeError);
  bad({ flux: 3 }, TypeError);
  assert.throws(() => m.getSignalHpss(signals[1], H, { harmonic: true }), TypeError);
  assert.throws(() => m.getSignalHpss(signals, 0, { harmonic: true }), RangeError);
  assert.deepStrictEqual(gathers(), []);
});

m.getSignalHpssAsync(signals, H, { flux: true, percussive: true }).then((r) => {
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'percussive', 'flux']);
  assert.strictEqual(mock.calls[mock.calls.length - 1].fn, 'hpssGatherAsync');
  n++;
  console.log('ok the async form');
  console.log('hpss_facade: ' + n + ' checks passed');
}).catch((e) => { console.error(e); process.exit(1); });
