'use strict';
// GPU check of getSignalOnsets / getSignalOnsetsAsync through the facade and the N-API addon: three signals (one
// without buffers); the onsets, their offsets and the envelope against the Python binding's (Plan.onsets, written by
// tests/test_js_onsets.py to DIR as raw files onsets.offsets.f64, onsets.peaks.f64 and onsets.envelope.f32), the async
// form against the synchronous one, the defaults, and the refusals. Needs an MI355X.
// usage: node onsets_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 1024, H = 256, NM = 40;
// (as tests/test_js_onsets.py asks for them)
const OPTS = { feature: 'melBands', mode: 'rectified', lag: 1, preMax: 3, postMax: 3, preAvg: 8, postAvg: 8, delta: 0.5, wait: 4 };
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
  const cuts = [0, 40 * N + 77, 40 * N + 77 + N - 1, x.length];
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: 44100 }, null, N, null, { numMelBands: NM });
  const r = m.getSignalOnsets(signals, H, Object.assign({ envelope: true }, OPTS));
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'onsetOffsets', 'onsets', 'envelope']);
  const batch = m.getBatchSignals('rms', signals, H);
  // the index arrays are of the type getBatchSignals gives frameOffsets
  assert.ok(r.onsetOffsets.constructor === batch.frameOffsets.constructor && r.onsets.constructor === batch.frameOffsets.constructor);
  sameBits(r.frameOffsets, batch.frameOffsets, 'frameOffsets');
  const F = r.frameOffsets[3];
  assert.ok(r.envelope instanceof Float32Array && r.envelope.length === F);
  assert.strictEqual(r.onsetOffsets.length, 4);
  assert.strictEqual(r.onsetOffsets[0], 0);
  assert.strictEqual(r.onsetOffsets[1], r.onsetOffsets[2]);  // the signal without buffers has no onsets
  assert.strictEqual(r.onsets.length, r.onsetOffsets[3]);
  assert.ok(r.onsetOffsets[1] > 2 && r.onsetOffsets[3] > r.onsetOffsets[2] + 2);
  for (let s = 0; s < 3; ++s) {
    for (let i = r.onsetOffsets[s]; i < r.onsetOffsets[s + 1]; ++i) {
      assert.ok(r.onsets[i] >= r.frameOffsets[s] && r.onsets[i] < r.frameOffsets[s + 1], 'onset ' + i + ' in its signal');
      if (i > r.onsetOffsets[s]) assert.ok(r.onsets[i] - r.onsets[i - 1] > OPTS.wait, 'onset ' + i + ' beyond wait');
    }
  }
  sameBits(r.onsetOffsets, expected('onsets.offsets.f64', Float64Array), 'onsetOffsets');
  sameBits(r.onsets, expected('onsets.peaks.f64', Float64Array), 'onsets');
  sameBits(r.envelope, expected('onsets.envelope.f32', Float32Array), 'envelope');
  console.log('ok onsets: the shapes, the empty signal, the Python binding\'s values');

  const ra = await m.getSignalOnsetsAsync(signals, H, Object.assign({ envelope: true }, OPTS));
  assert.deepStrictEqual(Object.keys(ra), Object.keys(r));
  for (const k of Object.keys(r)) sameBits(ra[k], r[k], 'async ' + k);
  console.log('ok the async form agrees');

  // without envelope the same onsets and no column; the defaults are mode 'rectified', lag 1 and zeros: with no
  // window, threshold or distance every buffer is an onset
  const bare = m.getSignalOnsets(signals, H, OPTS);
  assert.deepStrictEqual(Object.keys(bare), ['frameOffsets', 'onsetOffsets', 'onsets']);
  sameBits(bare.onsets, r.onsets, 'without envelope');
  const all = m.getSignalOnsets(signals, H, { feature: 'melBands' });
  sameBits(all.onsetOffsets, r.frameOffsets, 'defaults: offsets');
  assert.deepStrictEqual(Array.from(all.onsets), Array.from({ length: F }, (_, i) => i));
  // the envelope is getSignalSummaries' per-frame flux
  const fl = m.getSignalSummaries('rms', signals, H, { flux: [{ feature: 'melBands', perFrame: true }] });
  sameBits(r.envelope, fl.flux[0].perFrame, 'the flux call\'s column');
  console.log('ok the defaults, and the envelope is the flux call\'s');

  const bad = (o, E) => assert.throws(() => m.getSignalOnsets(signals, H, o), E);
  bad(undefined, TypeError);
  bad(3, TypeError);
  bad({}, TypeError);
  bad({ feature: 'rms' }, TypeError);
  bad({ feature: 'melBands', mode: 'l3' }, RangeError);
  for (const lag of [0, 9, 1.5, '2']) bad({ feature: 'melBands', lag }, RangeError);
  for (const k of ['preMax', 'postMax', 'preAvg', 'postAvg']) for (const v of [-1, 65, 1.5, '2']) bad({ feature: 'melBands', [k]: v }, RangeError);
  for (const wait of [-1, 4294967296, 0.5]) bad({ feature: 'melBands', wait }, RangeError);
  bad({ feature: 'melBands', delta: NaN }, RangeError);
  bad({ feature: 'melBands', delta: '1' }, TypeError);
  assert.throws(() => m.getSignalOnsets(x, H, OPTS), TypeError);
  m.dispose();
  console.log('onsets_gpu: 4 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
