'use strict';
// GPU checks of the facade's hopSize API through the N-API addon: getBatchSignal against getBatch on
// buffers cut in JavaScript, getBatchWav at a hop against getBatchSignal on the decoded channel, and the
// async forms against the sync ones -- element for element (Object.is: NaN for NaN, -0 for -0).
// Needs an MI355X.
const assert = require('assert');
const path = require('path');
const { wavS16 } = require('./wav');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const ctx = { sampleRate: 44100 };
const FEATS = ['rms', 'energy', 'zcr', 'spectralCentroid', 'spectralFlatness', 'spectralSlope', 'spectralRolloff',
  'spectralSpread', 'spectralSkewness', 'spectralKurtosis', 'loudness', 'perceptualSpread', 'perceptualSharpness', 'mfcc',
  'amplitudeSpectrum', 'complexSpectrum'];
let n = 0;
process.on('unhandledRejection', (e) => { console.error(e); process.exit(1); });

function same(a, b, what) {
  assert.deepStrictEqual(Object.keys(a).sort(), Object.keys(b).sort(), what);
  for (const k of Object.keys(b)) {
    assert.strictEqual(a[k].constructor, b[k].constructor, what + ' ' + k);
    assert.strictEqual(a[k].length, b[k].length, what + ' ' + k + ' length');
    for (let i = 0; i < b[k].length; i++) {
      if (!Object.is(a[k][i], b[k][i])) assert.fail(what + ' ' + k + '[' + i + ']: ' + a[k][i] + ' vs ' + b[k][i]);
    }
  }
}

// a seeded signal in [-1, 1) (an LCG: the same samples on every run)
function signal(S, seed) {
  const x = new Float32Array(S);
  let s = seed >>> 0;
  for (let i = 0; i < S; i++) {
    s = (Math.imul(s, 1664525) + 1013904223) >>> 0;
    x[i] = s / 2147483648 - 1;
  }
  return x;
}

function cut(x, N, H) {
  const F = Meyda.signalFrames(x.length, N, H);
  const frames = new Float32Array(F * N);
  for (let f = 0; f < F; f++) frames.set(x.subarray(f * H, f * H + N), f * N);
  return frames;
}

(async () => {
  const N = 512;
  const m = new Meyda(ctx, null, N);

  // getBatchSignal at hopSize = N / 2 against getBatch on buffers cut in JavaScript; a few buffers (one
  // launch over pinned memory) and enough for the chunked staging path
  for (const F of [1, 7, 700]) {
    const x = signal((F - 1) * (N / 2) + N + 100, 1234 + F);
    assert.strictEqual(Meyda.signalFrames(x.length, N, N / 2), F);
    const got = m.getBatchSignal(FEATS, x, N / 2);
    same(got, m.getBatch(FEATS, cut(x, N, N / 2)), 'getBatchSignal F=' + F);
    assert.strictEqual(got.rms.length, F);
    same(await m.getBatchSignalAsync(FEATS, x, N / 2), got, 'getBatchSignalAsync F=' + F);
  }
  n++;
  console.log('ok getBatchSignal equals getBatch on the cut buffers, sync and async');

  // a hop above N, and a signal shorter than one buffer
  {
    const x = signal(40 * N + 9, 77);
    same(m.getBatchSignal(FEATS, x, N + 3), m.getBatch(FEATS, cut(x, N, N + 3)), 'hop > N');
    const none = m.getBatchSignal(['rms', 'mfcc'], signal(N - 1, 5), 64);
    assert.strictEqual(none.rms.length, 0);
    assert.strictEqual(none.mfcc.length, 0);
  }
  n++;
  console.log('ok a hop above bufferSize, and no buffer at all');

  // getBatchWav(..., channel, hopSize) against getBatchSignal on the decoded channel (s16: v / 32768)
  {
    const S = 30 * N + 41, H = 200;
    const codes = new Int16Array(S * 2);
    const r = signal(S * 2, 99);
    for (let i = 0; i < codes.length; i++) codes[i] = Math.round(r[i] * 32767);
    const wav = wavS16(codes, 2, 44100);
    const chan = new Float32Array(S);
    for (let i = 0; i < S; i++) chan[i] = codes[2 * i + 1] / 32768;
    const got = m.getBatchWav(FEATS, wav, 1, H);
    assert.strictEqual(got.rms.length, Meyda.signalFrames(S, N, H));
    same(got, m.getBatchSignal(FEATS, chan, H), 'getBatchWav at a hop');
    same(await m.getBatchWavAsync(FEATS, wav, 1, H), got, 'getBatchWavAsync at a hop');
    // without hopSize: the disjoint buffers, i.e. hopSize = bufferSize
    same(m.getBatchWav(FEATS, wav, 1), m.getBatchSignal(FEATS, chan, N), 'getBatchWav without a hop');
  }
  n++;
  console.log('ok getBatchWav at a hop equals getBatchSignal on the decoded channel, sync and async');

  m.dispose();
  console.log('facade_signal_gpu: ' + n + ' checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
