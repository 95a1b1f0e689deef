'use strict';
// GPU checks of 'melBands' through the facade and the N-API addon: get(), getBatch, getBatchSignal and
// getBatchWav at a hop (sync and async) and the batched streaming callbacks on one signal with 40 bands. The
// rows are written to OUT_DIR as raw float32 files, which tests/test_js_melbands.py compares with the C ABI
// call's; here they are compared with each other. Needs an MI355X.
// usage: node melbands_gpu.js SIGNAL.f32 SIGNAL.wav OUT_DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, wavPath, outDir] = process.argv.slice(2);
const ctx = { sampleRate: 44100 };
const N = 1024, H = 256, NM = 40;
let n = 0;
process.on('unhandledRejection', (e) => { console.error(e); process.exit(1); });

function same(a, b, what) {
  assert.strictEqual(a.constructor, b.constructor, what);
  assert.strictEqual(a.length, b.length, what + ' length');
  for (let i = 0; i < b.length; i++) if (!Object.is(a[i], b[i])) assert.fail(what + '[' + i + ']: ' + a[i] + ' vs ' + b[i]);
}
function dump(name, a) {
  fs.writeFileSync(path.join(outDir, name), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  const wav = fs.readFileSync(wavPath);
  const m = new Meyda(ctx, null, N, null, { numMelBands: NM });
  assert.deepStrictEqual(m.featureInfo.melBands, { type: 'array' });
  const F = Meyda.signalFrames(x.length, N, H);

  // getBatchSignal(['melBands', 'mfcc'], x, 256), sync and async; melBands alone gives the same rows
  const sig = m.getBatchSignal(['melBands', 'mfcc'], x, H);
  assert.ok(sig.melBands instanceof Float32Array);
  assert.strictEqual(sig.melBands.length, F * NM);
  assert.strictEqual(sig.mfcc.length, F * 13);
  same(m.getBatchSignal('melBands', x, H).melBands, sig.melBands, 'melBands alone');
  const sigA = await m.getBatchSignalAsync(['melBands', 'mfcc'], x, H);
  same(sigA.melBands, sig.melBands, 'getBatchSignalAsync melBands');
  same(sigA.mfcc, sig.mfcc, 'getBatchSignalAsync mfcc');
  dump('signal_mel.f32', sig.melBands);
  dump('signal_mfcc.f32', sig.mfcc);
  n++;
  console.log('ok getBatchSignal returns melBands, sync and async');

  // get(['melBands']) and get('melBands') on buffer f of the signal: a Float32Array(40), row f
  for (const f of [0, 3, F - 1]) {
    m.process(x.slice(f * H, f * H + N));
    const g = m.get(['melBands', 'mfcc']);
    assert.ok(g.melBands instanceof Float32Array);
    assert.strictEqual(g.melBands.length, NM);
    same(g.melBands, sig.melBands.slice(f * NM, f * NM + NM), 'get melBands, buffer ' + f);
    same(m.get('melBands'), g.melBands, 'get string form');
    same(Meyda.frame(sig, 'melBands', f, N, 13, NM), g.melBands, 'Meyda.frame');
    if (f === 3) dump('get_mel_3.f32', g.melBands);
  }
  n++;
  console.log('ok get() returns a Float32Array(numMelBands) per buffer');

  // getBatch on the cut buffers, sync and async
  {
    const frames = new Float32Array(F * N);
    for (let f = 0; f < F; f++) frames.set(x.subarray(f * H, f * H + N), f * N);
    const b = m.getBatch(['melBands'], frames);
    same(b.melBands, sig.melBands, 'getBatch');
    same((await m.getBatchAsync(['melBands', 'rms'], frames)).melBands, sig.melBands, 'getBatchAsync');
  }
  n++;
  console.log('ok getBatch on the cut buffers');

  // getBatchWav at a hop (the file's channel 0 holds the signal as s16), sync and async, and without a hop
  {
    const w = m.getBatchWav(['melBands', 'mfcc'], wav, 0, H);
    assert.strictEqual(w.melBands.length, F * NM);
    same((await m.getBatchWavAsync(['melBands', 'mfcc'], wav, 0, H)).melBands, w.melBands, 'getBatchWavAsync');
    dump('wav_mel.f32', w.melBands);
    const d = m.getBatchWav('melBands', wav, 0);
    assert.strictEqual(d.melBands.length, Math.floor(x.length / N) * NM);
    dump('wav_dense_mel.f32', d.melBands);
  }
  n++;
  console.log('ok getBatchWav at a hop');

  // start() streaming, one callback per buffer, batched 4 at a time and one at a time
  for (const K of [1, 4]) {
    const rows = [];
    const s = new Meyda(ctx, null, N, (v) => rows.push(v.melBands), { numMelBands: NM, batchFrames: K });
    s.start(['melBands', 'rms']);
    for (let f = 0; f < 6; f++) s.process(x.slice(f * H, f * H + N));
    s.stop();
    assert.strictEqual(rows.length, 6);
    rows.forEach((r, f) => same(r, sig.melBands.slice(f * NM, f * NM + NM), 'streaming K=' + K + ' buffer ' + f));
    s.dispose();
  }
  n++;
  console.log('ok start() streaming delivers melBands per buffer');

  // options.devices: a clear error, as hopSize gives, before any device group is made
  {
    const g = new Meyda(ctx, null, N, null, { numMelBands: NM, devices: [0, 1] });
    for (const call of [() => g.getBatch(['melBands'], new Float32Array(N)), () => g.get('melBands'),
      () => g.getBatchSignal('melBands', x, H), () => g.getBatchWav(['mfcc', 'melBands'], wav, 0)]) {
      assert.throws(call, /melBands is not supported with options\.devices/);
    }
  }
  n++;
  console.log('ok options.devices throws');

  m.dispose();
  console.log('melbands_gpu: ' + n + ' checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
