'use strict';
// GPU checks of getBatchSignals / getBatchGather through the facade and the N-API addon: three signals in one
// call against per-signal getBatchSignal results, frameOffsets, the async forms, starts in any order, a start
// out of range, and options.devices. The concatenated rows are written to OUT_DIR as raw float32 files, which
// tests/test_js_gather.py compares with the C ABI call's. Needs an MI355X.
// usage: node gather_gpu.js SIGNAL.f32 OUT_DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, outDir] = process.argv.slice(2);
const ctx = { sampleRate: 44100 };
const N = 1024, H = 256, NM = 40;
const FEATS = ['rms', 'mfcc', 'melBands', 'loudness'];
let n = 0;
process.on('unhandledRejection', (e) => { console.error(e); process.exit(1); });

function same(a, b, what) {
  assert.strictEqual(a.constructor, b.constructor, what);
  assert.strictEqual(a.length, b.length, what + ' length');
  for (let i = 0; i < b.length; i++) if (!Object.is(a[i], b[i])) assert.fail(what + '[' + i + ']: ' + a[i] + ' vs ' + b[i]);
}
function sameResult(a, b, what) {
  const keys = (r) => Object.keys(r).filter((k) => k !== 'frameOffsets').sort();
  assert.deepStrictEqual(keys(a), keys(b), what);
  for (const k of keys(b)) same(a[k], b[k], what + ' ' + k);
}
function dump(name, a) {
  fs.writeFileSync(path.join(outDir, name), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
}

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  // three signals: a few buffers and a partial tail, fewer samples than one buffer, exactly two buffers at this hop
  const cuts = [0, 5 * N + 77, 5 * N + 77 + N - 1, 5 * N + 77 + N - 1 + N + H];
  assert.ok(x.length >= cuts[3]);
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda(ctx, null, N, null, { numMelBands: NM });
  const counts = signals.map((s) => Meyda.signalFrames(s.length, N, H));
  assert.deepStrictEqual(counts.slice(1), [0, 2]);

  const all = m.getBatchSignals(FEATS, signals, H);
  assert.ok(all.frameOffsets instanceof Float64Array);
  assert.deepStrictEqual(Array.from(all.frameOffsets), [0, counts[0], counts[0], counts[0] + 2]);
  const total = counts[0] + 2;
  assert.strictEqual(all.rms.length, total);
  assert.strictEqual(all.melBands.length, total * NM);
  for (const s of [0, 2]) {
    const one = m.getBatchSignal(FEATS, signals[s], H);
    const f0 = all.frameOffsets[s], f1 = all.frameOffsets[s + 1];
    for (const k of Object.keys(one)) {
      const w = one[k].length / (f1 - f0);
      same(all[k].slice(f0 * w, f1 * w), one[k], 'signal ' + s + ' ' + k);
    }
  }
  dump('signals_mel.f32', all.melBands);
  dump('signals_mfcc.f32', all.mfcc);
  n++;
  console.log('ok getBatchSignals equals per-signal getBatchSignal, frameOffsets right');

  const allA = await m.getBatchSignalsAsync(FEATS, signals, H);
  assert.deepStrictEqual(Array.from(allA.frameOffsets), Array.from(all.frameOffsets));
  sameResult(allA, all, 'getBatchSignalsAsync');
  n++;
  console.log('ok the async form agrees');

  // getBatchGather: the same buffers through the helper's starts, then backwards with a repeat
  {
    const t = Meyda.signalsFrameStarts(signals.map((s) => s.length), N, H);
    assert.deepStrictEqual(Array.from(t.frameOffsets), Array.from(all.frameOffsets));
    const cat = x.slice(0, cuts[3]);
    sameResult(m.getBatchGather(FEATS, cat, t.starts), all, 'getBatchGather');
    sameResult(await m.getBatchGatherAsync(FEATS, cat, Array.from(t.starts)), all, 'getBatchGatherAsync');
    const back = Array.from(t.starts).reverse().concat([t.starts[0]]);
    const r = m.getBatchGather(['rms', 'melBands'], cat, back);
    for (let f = 0; f < back.length; f++) {
      const g = f < total ? total - 1 - f : 0;
      assert.ok(Object.is(r.rms[f], all.rms[g]), 'reversed rms ' + f);
      same(r.melBands.slice(f * NM, f * NM + NM), all.melBands.slice(g * NM, g * NM + NM), 'reversed melBands ' + f);
    }
    assert.strictEqual(m.getBatchGather('rms', cat, []).rms.length, 0);
    assert.throws(() => m.getBatchGather('rms', cat, [cat.length - N + 1]), /starts\[0\]/);
    await assert.rejects(m.getBatchGatherAsync('rms', cat, [0, cat.length]), /starts\[1\]/);
  }
  n++;
  console.log('ok getBatchGather: any order, repeats, a start out of range refused');

  // options.devices: a clear error, as getBatchSignal gives, before any device group is made
  {
    const g = new Meyda(ctx, null, N, null, { devices: [0, 1] });
    assert.throws(() => g.getBatchSignals(['rms'], signals, H), /not supported with options\.devices/);
    assert.throws(() => g.getBatchSignalsAsync(['rms'], signals, H), /not supported with options\.devices/);
    assert.throws(() => g.getBatchGather(['rms'], x, [0]), /not supported with options\.devices/);
    assert.throws(() => g.getBatchGatherAsync(['rms'], x, [0]), /not supported with options\.devices/);
  }
  n++;
  console.log('ok options.devices throws');

  m.dispose();
  console.log('gather_gpu: ' + n + ' checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
