'use strict';
// Host-side checks of the facade's tempo plumbing (meyda.js getSignalTempo / getSignalTempoAsync) against a stand-in
// addon that records its calls (tests/js/tempo_addon.js): what reaches the addon, the defaults, the bpm arithmetic,
// the mean rows cut from the summary, and that a bad option never reaches it. The GPU results themselves:
// tests/js/tempo_gpu.js.
const path = require('path');
const assert = require('assert');
process.env.MEYDA_AMD_ADDON = path.join(__dirname, 'tempo_addon.js');
const mock = require('./tempo_addon');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

let n = 0;
function check(name, fn) { fn(); n++; console.log('ok ' + name); }
const N = 256, H = 64, SR = 44100;
const m = new Meyda({ sampleRate: SR }, null, N);
const signals = [new Float32Array(N - 1), new Float32Array(N + 9 * H), new Float32Array(N), new Float32Array(N + 2 * H + 5)];

check('the defaults reach the addon', () => {
  mock.calls.length = 0;
  const r = m.getSignalTempo(signals, { hopSize: H });
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['tempogramWindow', 'tempoPrior', 'tempoGather']);
  assert.deepStrictEqual(mock.calls[0].args, [384]);
  assert.deepStrictEqual(mock.calls[1].args, [SR / H, 384, { startBpm: 120, stdOctaves: 1, maxBpm: 320 }]);
  const [samples, starts, fo, o] = mock.calls[2].args;
  assert.strictEqual(samples.length, signals.reduce((a, x) => a + x.length, 0));
  assert.deepStrictEqual(Array.from(fo), [0, 0, 10, 11, 14]);
  assert.strictEqual(starts.length, 14);
  assert.deepStrictEqual(Object.keys(o), ['field', 'mode', 'lag', 'winLength', 'numLags', 'norm', 'gain', 'window', 'prior', 'mean', 'envelope']);
  assert.deepStrictEqual([o.field, o.mode, o.lag, o.winLength, o.numLags, o.norm, o.gain, o.mean, o.envelope], [19, 0, 1, 384, 384, 1, 1e6, false, false]);
  assert.ok(o.window instanceof Float32Array && o.window.length === 384 && o.prior instanceof Float64Array && o.prior.length === 384);
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags']);
  assert.ok(r.lag instanceof Uint32Array && r.bpm instanceof Float64Array && r.numLags === 384);
});

check('the bpm arithmetic', () => {
  const r = m.getSignalTempo(signals, { hopSize: H });
  assert.deepStrictEqual(Array.from(r.lag), [0, 86, 43, 7]);
  assert.ok(Number.isNaN(r.bpm[0]));
  for (const s of [1, 2, 3]) assert.strictEqual(r.bpm[s], 60 * (SR / H) / r.lag[s]);
  const at256 = new Meyda({ sampleRate: SR }, null, 1024).getSignalTempo([new Float32Array(4096), new Float32Array(4096)], { hopSize: 256 });
  assert.ok(Math.abs(at256.bpm[1] - 120.19) < 0.005);  // lag 86 at 172.27 rows a second
});

check('the options reach the addon in the library\'s numbers', () => {
  mock.calls.length = 0;
  const window = new Float32Array(64).fill(1), prior = new Float64Array(48).fill(1);
  const r = m.getSignalTempo(signals, { hopSize: 32, feature: 'amplitudeSpectrum', mode: 'l2', lag: 3, winLength: 64, numLags: 48, norm: 'none',
    gain: 10, window, prior, mean: true, envelope: true, startBpm: 90 });
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['tempoGather']);  // the caller's window and prior: none is built
  const o = mock.calls[0].args[3];
  assert.deepStrictEqual([o.field, o.mode, o.lag, o.winLength, o.numLags, o.norm, o.gain, o.mean, o.envelope], [15, 2, 3, 64, 48, 0, 10, true, true]);
  assert.ok(o.window === window && o.prior === prior);
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags', 'mean', 'envelope']);
  // the mean rows are statistic 0 of every signal's summary
  assert.ok(r.mean instanceof Float64Array && r.mean.length === 4 * 48);
  for (let s = 0; s < 4; ++s) for (const l of [0, 1, 47]) assert.strictEqual(r.mean[s * 48 + l], 1000 * s + l);
  assert.strictEqual(r.bpm[1], 60 * (SR / 32) / 86);
  // numLags defaults to winLength; the prior's options go to tempoPrior
  mock.calls.length = 0;
  m.getSignalTempo(signals, { hopSize: H, winLength: 100, startBpm: 90, stdOctaves: 0.5, maxBpm: 0 });
  assert.deepStrictEqual(mock.calls[0].args, [100]);
  assert.deepStrictEqual(mock.calls[1].args, [SR / H, 100, { startBpm: 90, stdOctaves: 0.5, maxBpm: 0 }]);
  assert.strictEqual(mock.calls[2].args[3].numLags, 100);
});

check('a bad option never reaches the addon', () => {
  mock.calls.length = 0;
  const bad = (o, E) => assert.throws(() => m.getSignalTempo(signals, o), E);
  bad(undefined, TypeError);
  bad(3, TypeError);
  for (const hopSize of [undefined, 0, -1, 1.5, '64']) bad({ hopSize }, RangeError);
  bad({ hopSize: H, feature: 'rms' }, TypeError);
  bad({ hopSize: H, mode: 'l3' }, RangeError);
  for (const lag of [0, 9, 1.5]) bad({ hopSize: H, lag }, RangeError);
  for (const winLength of [0, 1, 1025, 2.5, '384']) bad({ hopSize: H, winLength }, RangeError);
  for (const numLags of [0, 385, 1.5]) bad({ hopSize: H, numLags }, RangeError);
  bad({ hopSize: H, norm: 'max' }, RangeError);
  for (const gain of [-1, Infinity, NaN, '1']) bad({ hopSize: H, gain }, RangeError);
  bad({ hopSize: H, window: new Float32Array(10) }, TypeError);
  bad({ hopSize: H, window: new Float64Array(384) }, TypeError);
  bad({ hopSize: H, prior: new Float32Array(384) }, TypeError);
  bad({ hopSize: H, prior: new Float64Array(383) }, TypeError);
  for (const startBpm of [0, -1, Infinity, NaN, '120']) bad({ hopSize: H, startBpm }, RangeError);
  for (const stdOctaves of [0, -1, NaN]) bad({ hopSize: H, stdOctaves }, RangeError);
  for (const maxBpm of [-1, Infinity, NaN]) bad({ hopSize: H, maxBpm }, RangeError);
  assert.throws(() => m.getSignalTempo(new Float32Array(10), { hopSize: H }), TypeError);
  assert.deepStrictEqual(mock.calls.filter((c) => c.fn.startsWith('tempoGather')), []);
  for (const W of [1, 1025, 2.5, '8']) assert.throws(() => Meyda.tempogramWindow(W), RangeError);
  for (const rate of [0, -1, Infinity, NaN, '100']) assert.throws(() => Meyda.tempoPrior(rate, 8), RangeError);
  for (const L of [0, 1025, 1.5]) assert.throws(() => Meyda.tempoPrior(100, L), RangeError);
  assert.throws(() => Meyda.tempoPrior(100, 8, 3), TypeError);
});

m.getSignalTempoAsync(signals, { hopSize: H, mean: true }).then((r) => {
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags', 'mean']);
  assert.deepStrictEqual(Array.from(r.lag), [0, 86, 43, 7]);
  assert.strictEqual(mock.calls[mock.calls.length - 1].fn, 'tempoGatherAsync');
  n++;
  console.log('ok the async form');
  console.log('tempo_facade: ' + n + ' checks passed');
}).catch((e) => { console.error(e); process.exit(1); });
