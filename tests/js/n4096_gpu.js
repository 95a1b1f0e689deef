'use strict';
// GPU checks of bufferSize 4096 through the facade and the N-API addon: `new Meyda(ctx, null, 4096)`, get() of a
// few features on buffers of one signal and getBatchSignal at hop 1024. The values are written to OUT_DIR as raw
// files, which tests/test_js_n4096.py compares with the C ABI call's; here they are compared with each other.
// A size above the range throws the library's message; one that is no power of two throws the reference's.
// Needs an MI355X.   usage: node n4096_gpu.js SIGNAL.f32 OUT_DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, outDir] = process.argv.slice(2);
const ctx = { sampleRate: 44100 };
const N = 4096, H = 1024;
const FEATS = ['rms', 'zcr', 'spectralCentroid', 'spectralRolloff', 'mfcc', 'loudness', 'amplitudeSpectrum'];
let n = 0;
process.on('unhandledRejection', (e) => { console.error(e); process.exit(1); });

function same(a, b, what) {
  assert.strictEqual(a.length, b.length, what + ' length');
  for (let i = 0; i < b.length; i++) if (!Object.is(a[i], b[i])) assert.fail(what + '[' + i + ']: ' + a[i] + ' vs ' + b[i]);
}
function dump(name, a) {
  fs.writeFileSync(path.join(outDir, name), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));

  // the reference's order: the power-of-two check first (src/meyda.js:20-26), then the library's range
  assert.throws(() => new Meyda(ctx, null, 4095), /Buffer size is not a power of two: Meyda will not run\./);
  assert.throws(() => { const big = new Meyda(ctx, null, 8192); big.getBatch(['rms'], new Float32Array(8192)); }, /256\.\.4096/);
  n++;
  console.log('ok 4095 throws the reference\'s error, 8192 the library\'s range');

  const m = new Meyda(ctx, null, N);
  const F = Meyda.signalFrames(x.length, N, H);
  const sig = m.getBatchSignal(FEATS, x, H);
  assert.strictEqual(sig.rms.length, F);
  assert.strictEqual(sig.amplitudeSpectrum.length, F * (N / 2));
  assert.strictEqual(sig.mfcc.length, F * 13);
  const sigA = await m.getBatchSignalAsync(FEATS, x, H);
  for (const k of Object.keys(sig)) {
    if (sig[k] && sig[k].length !== undefined) same(sigA[k], sig[k], 'getBatchSignalAsync ' + k);
  }
  dump('signal_rms.bin', sig.rms);
  dump('signal_centroid.bin', sig.spectralCentroid);
  dump('signal_mfcc.f32', sig.mfcc);
  dump('signal_amp.f32', sig.amplitudeSpectrum);
  fs.writeFileSync(path.join(outDir, 'scalar_bytes.txt'), String(sig.rms.BYTES_PER_ELEMENT));
  n++;
  console.log('ok getBatchSignal at hop 1024, sync and async');

  // get([...]) on buffer f of the signal: row f of the batch
  for (const f of [0, 2, F - 1]) {
    m.process(x.slice(f * H, f * H + N));
    const g = m.get(['rms', 'spectralCentroid', 'mfcc', 'amplitudeSpectrum']);
    assert.strictEqual(g.amplitudeSpectrum.length, N / 2);
    assert.strictEqual(g.mfcc.length, 13);
    same(g.amplitudeSpectrum, sig.amplitudeSpectrum.slice(f * (N / 2), (f + 1) * (N / 2)), 'get amplitudeSpectrum, buffer ' + f);
    same(g.mfcc, sig.mfcc.slice(f * 13, f * 13 + 13), 'get mfcc, buffer ' + f);
    if (f === 2) {
      dump('get_amp_2.f32', Float32Array.from(g.amplitudeSpectrum));
      dump('get_mfcc_2.f32', Float32Array.from(g.mfcc));
      dump('get_scalars_2.f64', Float64Array.from([g.rms, g.spectralCentroid]));
    }
  }
  n++;
  console.log('ok get() on buffers of the signal');

  m.dispose();
  console.log('n4096_gpu: ' + n + ' checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
