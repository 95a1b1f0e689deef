'use strict';
// GPU check of getSignalChroma / getSignalChromaAsync through the facade and the N-API addon: three signals (one
// without buffers); the chroma rows and their summaries against the Python binding's (Plan.chroma_signals, written by
// tests/test_js_chroma_gpu.py to DIR as raw files chroma.rows.f32, chroma.STAT.f64 and chroma13.rows.f32), the async
// form against the synchronous one, a caller's bank, the defaults, and the refusals. Needs an MI355X.
// usage: node chroma_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 1024, H = 256;
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
  const cuts = [0, 5 * N + 77, 5 * N + 77 + N - 1, x.length];
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: 44100 }, null, N, null, {});
  const r = m.getSignalChroma(signals, H, { summary: true });
  assert.deepStrictEqual(Object.keys(r), ['chroma', 'numChroma', 'frameOffsets', 'summaries']);
  const batch = m.getBatchSignals('rms', signals, H);
  sameBits(r.frameOffsets, batch.frameOffsets, 'frameOffsets');
  const F = r.frameOffsets[3];
  assert.strictEqual(r.numChroma, 12);
  assert.ok(r.chroma instanceof Float32Array && r.chroma.length === F * 12);
  for (let t = 0; t < F; ++t) assert.strictEqual(Math.max.apply(null, r.chroma.subarray(t * 12, t * 12 + 12)), 1);
  sameBits(r.chroma, expected('chroma.rows.f32', Float32Array), 'chroma');
  assert.deepStrictEqual(Object.keys(r.summaries), ['mean', 'variance', 'min', 'max']);
  for (const k of Object.keys(r.summaries)) {
    assert.ok(r.summaries[k] instanceof Float64Array && r.summaries[k].length === 3 * 12);
    for (let c = 0; c < 12; ++c) assert.ok(Number.isNaN(r.summaries[k][12 + c]), 'the signal without buffers is NaN');
    sameBits(r.summaries[k], expected('chroma.' + k + '.f64', Float64Array), 'summaries.' + k);
  }
  console.log('ok chroma: the shapes, the empty signal, the Python binding\'s values');

  const ra = await m.getSignalChromaAsync(signals, H, { summary: true });
  assert.deepStrictEqual(Object.keys(ra), Object.keys(r));
  sameBits(ra.chroma, r.chroma, 'async chroma');
  for (const k of Object.keys(r.summaries)) sameBits(ra.summaries[k], r.summaries[k], 'async ' + k);
  console.log('ok the async form agrees');

  // without options: the rows alone, the same; the bank the call builds is Meyda.chromaFilterBank's
  const bare = m.getSignalChroma(signals, H);
  assert.deepStrictEqual(Object.keys(bare), ['chroma', 'numChroma', 'frameOffsets']);
  sameBits(bare.chroma, r.chroma, 'without options');
  const own = m.getSignalChroma(signals, H, { weights: Meyda.chromaFilterBank(N, 44100) });
  sameBits(own.chroma, r.chroma, 'the bank handed in');
  // 13 rows without octave weighting, row 0 at A, unnormalised: the Python binding's
  const o13 = { numChroma: 13, octaveWidth: 0, baseC: false, norm: 'none' };
  const r13 = m.getSignalChroma(signals, H, o13);
  assert.strictEqual(r13.numChroma, 13);
  sameBits(r13.chroma, expected('chroma13.rows.f32', Float32Array), '13 rows, norm none');
  // chroma flux, the harmonic-change envelope, needs no more than the rows: they are ordinary float32 rows
  assert.ok(r13.chroma.every((v) => Number.isFinite(v) && v > 0));
  console.log('ok the defaults, a bank handed in, 13 rows unnormalised');

  const bad = (o, E) => assert.throws(() => m.getSignalChroma(signals, H, o), E);
  bad(3, TypeError);
  bad({ norm: 'l2' }, RangeError);
  bad({ weights: [1, 2, 3] }, TypeError);
  bad({ weights: new Float32Array(100) }, RangeError);
  bad({ weights: new Float32Array(12 * N / 2), numChroma: 13 }, RangeError);
  bad({ weights: new Float32Array(37 * N / 2) }, RangeError);
  for (const numChroma of [0, 37, 1.5, '12']) bad({ numChroma }, RangeError);
  bad({ a440: 0 }, RangeError);
  bad({ octaveWidth: -1 }, RangeError);
  assert.throws(() => m.getSignalChroma(x, H), TypeError);
  assert.throws(() => m.getSignalChroma(signals, 0), RangeError);
  // the addon's own checks, past the facade's
  const st = Meyda.signalsFrameStarts(signals.map((s) => s.length), N, H);
  assert.throws(() => Meyda.addon.chromaGather(m._plan(), x, st.starts, st.frameOffsets, { numChroma: 12 }), TypeError);
  assert.throws(() => Meyda.addon.chromaGather(m._plan(), x, st.starts, null, { numChroma: 12, weights: Meyda.chromaFilterBank(N, 44100), summary: true }), RangeError);
  m.dispose();
  console.log('chroma_gpu: 4 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
