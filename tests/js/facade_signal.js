'use strict';
// Host-side checks of the facade's hopSize plumbing (meyda.js getBatchSignal / getBatchWav /
// Meyda.signalFrames) against a stand-in addon that records its calls (tests/js/signal_addon.js): what
// reaches the addon, that a bad hopSize never does, and that device groups refuse a hop. Then
// Meyda.signalFrames through the real addon, when it is built (mgx_signal_frames needs no GPU). The GPU
// results themselves: tests/js/facade_signal_gpu.js.
const fs = require('fs');
const path = require('path');
const assert = require('assert');
const MEYDA = path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js');
const REAL = path.join(__dirname, '..', '..', 'meyda_amd', 'addon', 'meyda_napi.node');
process.env.MEYDA_AMD_ADDON = path.join(__dirname, 'signal_addon.js');
const mock = require('./signal_addon');
const Meyda = require(MEYDA);

const ctx = { sampleRate: 44100 };
let n = 0;
function check(name, fn) { fn(); n++; console.log('ok ' + name); }
const N = 256;
const formula = (S, B, H) => (S < B ? 0 : Math.floor((S - B) / H) + 1);
const CASES = [];
for (const B of [256, 2048]) {
  for (const H of [1, 63, B / 4, B, B + 1, 5 * B]) {
    for (const S of [0, B - 1, B, B + 1, B + H - 1, B + H, 10 * B + 7]) CASES.push([S, B, H]);
  }
}
CASES.push([2 ** 40, 1024, 1]);

check('getBatchSignal forwards the samples, hopSize and names unchanged', () => {
  const m = new Meyda(ctx, null, N);
  const x = new Float32Array(5 * N + 3);
  mock.calls.length = 0;
  m.getBatchSignal(['rms', 'mfcc'], x, 64);
  assert.strictEqual(mock.calls.length, 1);
  const c = mock.calls[0];
  assert.strictEqual(c.fn, 'extractSignal');
  assert.strictEqual(c.args[1], x);
  assert.strictEqual(c.args[2], 64);
  assert.deepStrictEqual(c.args[3], ['rms', 'mfcc']);
  assert.strictEqual(c.args.length, 4);
  mock.calls.length = 0;
  m.getBatchSignal('rms', Array.from({ length: 300 }, () => 0.5), N + 1);  // (a plain array is converted)
  assert.ok(mock.calls[0].args[1] instanceof Float32Array);
  assert.strictEqual(mock.calls[0].args[2], N + 1);
});

check('getBatchWav forwards hopSize, and without it makes the call it always made', () => {
  const m = new Meyda(ctx, null, N);
  const wav = Buffer.alloc(64);
  mock.calls.length = 0;
  m.getBatchWav(['rms'], wav, 1, 128);
  m.getBatchWav(['rms'], wav, 1);
  m.getBatchWav(['rms'], wav);
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['extractWav', 'extractWav', 'extractWav']);
  assert.deepStrictEqual(mock.calls[0].args.slice(1), [wav, ['rms'], 1, 128]);
  assert.deepStrictEqual(mock.calls[1].args.slice(1), [wav, ['rms'], 1]);
  assert.deepStrictEqual(mock.calls[2].args.slice(1), [wav, ['rms'], 0]);
});

check('a bad hopSize is a RangeError before the addon is called', () => {
  const m = new Meyda(ctx, null, N);
  const x = new Float32Array(4 * N);
  m.getBatchSignal(['rms'], x, N);  // (the plan exists from here on)
  mock.calls.length = 0;
  for (const bad of [0, -1, 1.5, 'a', NaN, null, 2 ** 32]) {
    assert.throws(() => m.getBatchSignal(['rms'], x, bad), RangeError, String(bad));
    assert.throws(() => m.getBatchSignalAsync(['rms'], x, bad), RangeError, String(bad));
    assert.throws(() => m.getBatchWav(['rms'], Buffer.alloc(64), 0, bad), RangeError, String(bad));
    assert.throws(() => m.getBatchWavAsync(['rms'], Buffer.alloc(64), 0, bad), RangeError, String(bad));
    assert.throws(() => Meyda.signalFrames(4096, N, bad), RangeError, String(bad));
  }
  assert.throws(() => m.getBatchSignal(['rms'], x), RangeError);  // (no hopSize at all)
  assert.strictEqual(mock.calls.length, 0);
});

check('an instance with options.devices refuses a hop, naming the option', () => {
  const m = new Meyda(ctx, null, N, null, { devices: [0, 1] });
  mock.calls.length = 0;
  assert.throws(() => m.getBatchSignal(['rms'], new Float32Array(4 * N), 64), /options\.devices/);
  assert.throws(() => m.getBatchSignalAsync(['rms'], new Float32Array(4 * N), 64), /options\.devices/);
  assert.throws(() => m.getBatchWav(['rms'], Buffer.alloc(64), 0, 64), /options\.devices/);
  assert.throws(() => m.getBatchWavAsync(['rms'], Buffer.alloc(64), 0, 64), /options\.devices/);
  assert.strictEqual(mock.calls.length, 0);
  m.getBatchWav(['rms'], Buffer.alloc(64), 0);  // (without a hop: today's call, groups included)
  assert.strictEqual(mock.calls.length, 1);
});

check('Meyda.signalFrames passes its arguments on', () => {
  mock.calls.length = 0;
  for (const [S, B, H] of CASES) assert.strictEqual(Meyda.signalFrames(S, B, H), formula(S, B, H), [S, B, H].join());
  assert.deepStrictEqual(mock.calls[0], { fn: 'signalFrames', args: CASES[0] });
});

(async () => {
  const m = new Meyda(ctx, null, N);
  const x = new Float32Array(3 * N);
  mock.calls.length = 0;
  await m.getBatchSignalAsync(['zcr'], x, 32);
  await m.getBatchWavAsync(['zcr'], Buffer.alloc(64), 1, 32);
  await m.getBatchWavAsync(['zcr'], Buffer.alloc(64), 1);
  assert.deepStrictEqual(mock.calls.map((c) => c.fn), ['extractSignalAsync', 'extractWavAsync', 'extractWavAsync']);
  assert.deepStrictEqual(mock.calls[0].args.slice(1), [x, 32, ['zcr']]);
  assert.deepStrictEqual(mock.calls[1].args.slice(3), [1, 32]);
  assert.deepStrictEqual(mock.calls[2].args.slice(3), [1]);
  n++;
  console.log('ok the async forms forward the same arguments');

  // the real addon, when built: mgx_signal_frames itself behind Meyda.signalFrames
  if (fs.existsSync(REAL)) {
    delete require.cache[require.resolve(MEYDA)];
    delete process.env.MEYDA_AMD_ADDON;
    const Real = require(MEYDA);
    assert.strictEqual(typeof Real.addon.abiVersion, 'function');
    for (const [S, B, H] of CASES) assert.strictEqual(Real.signalFrames(S, B, H), formula(S, B, H), [S, B, H].join());
    assert.throws(() => Real.addon.signalFrames(4096, 256, 0), /hop/);
    console.log('ok Meyda.signalFrames agrees with the formula through the real addon');
  } else {
    console.log('skip the real addon is not built');
  }
  console.log('facade_signal: ' + n + ' checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
