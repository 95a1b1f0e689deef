'use strict';
// Host-side checks of the facade's beat plumbing (meyda.js getSignalBeats / getSignalBeatsAsync) against a stand-in
// addon that records its calls (tests/js/beats_addon.js): what reaches the addon, the defaults, the per-signal lists,
// and that a bad option never reaches it. The GPU results themselves: tests/js/beats_gpu.js.
const path = require('path');
const assert = require('assert');
process.env.MEYDA_AMD_ADDON = path.join(__dirname, 'beats_addon.js');
const mock = require('./beats_addon');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

let n = 0;
function check(name, fn) { fn(); n++; console.log('ok ' + name); }
const N = 256, H = 64, SR = 44100;
const m = new Meyda({ sampleRate: SR }, null, N);
const signals = [new Float32Array(N - 1), new Float32Array(N + 9 * H), new Float32Array(N), new Float32Array(N + 2 * H + 5)];

check('the defaults reach the addon', () => {
  mock.calls.length = 0;
  const r = m.getSignalBeats(signals, { hopSize: H });
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['tempogramWindow', 'tempoPrior', 'beatTables', 'beatsGather']);
  assert.deepStrictEqual(mock.calls[2].args, [383, 100]);
  const [samples, starts, fo, o] = mock.calls[3].args;
  assert.strictEqual(samples.length, signals.reduce((a, x) => a + x.length, 0));
  assert.deepStrictEqual(Array.from(fo), [0, 0, 10, 11, 14]);
  assert.strictEqual(starts.length, 14);
  assert.deepStrictEqual(Object.keys(o), ['field', 'mode', 'lag', 'winLength', 'numLags', 'norm', 'gain', 'window', 'prior', 'envelope',
    'maxPeriod', 'trim', 'gauss', 'penalty']);
  assert.deepStrictEqual([o.field, o.mode, o.lag, o.winLength, o.numLags, o.norm, o.gain, o.envelope, o.maxPeriod, o.trim],
    [19, 0, 1, 384, 384, 1, 1e6, false, 383, true]);
  assert.ok(o.gauss instanceof Float32Array && o.gauss.length === 384 * 385 / 2 && o.penalty instanceof Float64Array && o.penalty.length === 384 * 384);
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags', 'beatOffsets', 'beats', 'signals']);
});

check('the lag, the bpm and the beats of every signal', () => {
  const r = m.getSignalBeats(signals, { hopSize: H });
  assert.deepStrictEqual(Array.from(r.lag), [0, 86, 43, 7]);
  assert.deepStrictEqual(Array.from(r.beatOffsets), [0, 0, 2, 2, 4]);
  assert.deepStrictEqual(Array.from(r.beats), [1, 2, 12, 13]);
  assert.strictEqual(r.signals.length, 4);
  assert.deepStrictEqual(r.signals.map((s) => Array.from(s.beats)), [[], [1, 2], [], [1, 2]]);  // from each signal's own first buffer
  assert.ok(Number.isNaN(r.signals[0].bpm) && r.signals[0].lag === 0);
  for (const s of [1, 2, 3]) assert.ok(r.signals[s].lag === r.lag[s] && r.signals[s].bpm === 60 * (SR / H) / r.lag[s]);
});

check('the options reach the addon in the library\'s numbers', () => {
  mock.calls.length = 0;
  const window = new Float32Array(64).fill(1), prior = new Float64Array(48).fill(1);
  const tables = Meyda.beatTables(60, 50);
  mock.calls.length = 0;
  const r = m.getSignalBeats(signals, { hopSize: 32, feature: 'amplitudeSpectrum', mode: 'l2', lag: 3, winLength: 64, numLags: 48, norm: 'none',
    gain: 10, window, prior, envelope: true, maxPeriod: 60, trim: false, tables });
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['beatsGather']);  // the caller's window, prior and tables: none is built
  const o = mock.calls[0].args[3];
  assert.deepStrictEqual([o.field, o.mode, o.lag, o.winLength, o.numLags, o.norm, o.gain, o.envelope, o.maxPeriod, o.trim],
    [15, 2, 3, 64, 48, 0, 10, true, 60, false]);
  assert.ok(o.window === window && o.prior === prior && o.gauss === tables.gauss && o.penalty === tables.penalty);
  assert.ok(r.envelope instanceof Float32Array);
  // maxPeriod defaults to numLags - 1 and the tightness goes to beatTables
  mock.calls.length = 0;
  m.getSignalBeats(signals, { hopSize: H, winLength: 100, tightness: 400 });
  assert.deepStrictEqual(mock.calls[2].args, [99, 400]);
  assert.strictEqual(mock.calls[3].args[3].maxPeriod, 99);
});

check('a bad option never reaches the addon', () => {
  mock.calls.length = 0;
  const bad = (o, E) => assert.throws(() => m.getSignalBeats(signals, o), E);
  bad(undefined, TypeError);
  for (const hopSize of [undefined, 0, 1.5]) bad({ hopSize }, RangeError);
  bad({ hopSize: H, feature: 'rms' }, TypeError);
  bad({ hopSize: H, winLength: 1025 }, RangeError);
  bad({ hopSize: H, mean: true }, TypeError);
  for (const maxPeriod of [0, 382, 1024, 400.5, '500']) bad({ hopSize: H, maxPeriod }, RangeError);
  for (const tightness of [0, -1, Infinity, NaN, '100']) bad({ hopSize: H, tightness }, RangeError);
  bad({ hopSize: H, tables: 3 }, TypeError);
  bad({ hopSize: H, tables: { gauss: new Float32Array(3), penalty: new Float64Array(4) } }, TypeError);
  bad({ hopSize: H, maxPeriod: 500, tables: Meyda.beatTables(383) }, TypeError);
  assert.deepStrictEqual(mock.calls.filter((c) => c.fn.startsWith('beatsGather')), []);
  for (const P of [0, 1024, 2.5, '8']) assert.throws(() => Meyda.beatTables(P), RangeError);
  for (const t of [0, -1, NaN, '1']) assert.throws(() => Meyda.beatTables(8, t), RangeError);
});

m.getSignalBeatsAsync(signals, { hopSize: H }).then((r) => {
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags', 'beatOffsets', 'beats', 'signals']);
  assert.deepStrictEqual(Array.from(r.beats), [1, 2, 12, 13]);
  assert.strictEqual(mock.calls[mock.calls.length - 1].fn, 'beatsGatherAsync');
  n++;
  console.log('ok the async form');
  console.log('beats_facade: ' + n + ' checks passed');
}).catch((e) => { console.error(e); process.exit(1); });
