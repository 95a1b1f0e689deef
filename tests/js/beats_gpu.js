'use strict';
// GPU check of getSignalBeats / getSignalBeatsAsync through the facade and the N-API addon: three signals (one without
// buffers); the lags, the beat lists and the envelope against the Python binding's (Plan.beats_signals, written by
// tests/test_js_beats_gpu.py to DIR as raw files beats.lag.u32, beats.offsets.u64, beats.rows.u64,
// beats.envelope.f32 and, without the trim, loose.rows.u64), the per-signal lists, the async form against the
// synchronous one, tables handed in, and the addon's own refusals. Needs an MI355X.
// usage: node beats_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 256, H = 64, SR = 44100;
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
// (row indices: 64-bit in the binding's files, Float64Arrays here)
const rowsOf = (name) => Float64Array.from(expected(name, BigUint64Array), (v) => Number(v));

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  const cuts = [0, 600 * H + N + 7, 600 * H + N + 7 + N - 1, x.length];
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: SR }, null, N, null, { numMelBands: 40 });
  const PRIOR = { startBpm: 1722.65625, maxBpm: 0 };
  const opts = Object.assign({ hopSize: H, winLength: 64, numLags: 48, envelope: true }, PRIOR);
  const r = m.getSignalBeats(signals, opts);
  assert.deepStrictEqual(Object.keys(r), ['frameOffsets', 'lag', 'bpm', 'numLags', 'envelope', 'beatOffsets', 'beats', 'signals']);
  const batch = m.getBatchSignals('rms', signals, H);
  sameBits(r.frameOffsets, batch.frameOffsets, 'frameOffsets');
  sameBits(r.lag, expected('beats.lag.u32', Uint32Array), 'lag');
  sameBits(r.beatOffsets, rowsOf('beats.offsets.u64'), 'beatOffsets');
  sameBits(r.beats, rowsOf('beats.rows.u64'), 'beats');
  sameBits(r.envelope, expected('beats.envelope.f32', Float32Array), 'envelope');
  // the signal without buffers: no tempo and no beats; the others: beats inside their own buffers, ascending
  assert.ok(r.lag[1] === 0 && r.signals[1].beats.length === 0 && Number.isNaN(r.signals[1].bpm));
  for (const s of [0, 2]) {
    const b = r.signals[s].beats, F = r.frameOffsets[s + 1] - r.frameOffsets[s];
    assert.ok(b.length > 5 && b[0] >= 0 && b[b.length - 1] < F && r.signals[s].lag === r.lag[s]);
    for (let i = 0; i < b.length; ++i) assert.strictEqual(b[i] + r.frameOffsets[s], r.beats[r.beatOffsets[s] + i]);
    for (let i = 1; i < b.length; ++i) assert.ok(b[i] > b[i - 1]);
    assert.strictEqual(r.signals[s].bpm, 60 * (SR / H) / r.lag[s]);
  }
  console.log('ok beats: the shapes, the empty signal, the Python binding\'s values, the per-signal lists');

  const ra = await m.getSignalBeatsAsync(signals, opts);
  assert.deepStrictEqual(Object.keys(ra), Object.keys(r));
  for (const k of ['lag', 'bpm', 'envelope', 'beatOffsets', 'beats']) sameBits(ra[k], r[k], 'async ' + k);
  console.log('ok the async form agrees');

  // tables handed in (a larger maxPeriod holds the same rows for these periods), and no trim
  const own = m.getSignalBeats(signals, Object.assign({}, opts, { maxPeriod: 100, tables: Meyda.beatTables(100) }));
  sameBits(own.beats, r.beats, 'tables handed in');
  const loose = m.getSignalBeats(signals, Object.assign({}, opts, { trim: false }));
  sameBits(loose.beats, rowsOf('loose.rows.u64'), 'trim false');
  console.log('ok tables handed in, no trim');

  // the addon's own checks, past the facade's
  const st = Meyda.signalsFrameStarts(signals.map((s) => s.length), N, H);
  const w = Meyda.tempogramWindow(64), p = Meyda.tempoPrior(SR / H, 48), t = Meyda.beatTables(47);
  const ok = { field: 19, winLength: 64, numLags: 48, window: w, prior: p, gauss: t.gauss, penalty: t.penalty };
  const call = (o, fo) => Meyda.addon.beatsGather(m._plan(), x, st.starts, fo === undefined ? st.frameOffsets : fo, o);
  assert.ok(call(ok).beats instanceof Float64Array);
  assert.throws(() => call(Object.assign({}, ok, { gauss: undefined })), TypeError);
  assert.throws(() => call(Object.assign({}, ok, { penalty: new Float32Array(48 * 48) })), TypeError);
  assert.throws(() => call(Object.assign({}, ok, { maxPeriod: 46 })), RangeError);   // a lag may reach 47
  assert.throws(() => call(Object.assign({}, ok, { maxPeriod: 48 })), RangeError);   // the tables' lengths
  assert.throws(() => call(Object.assign({}, ok, { maxPeriod: 1024 })), RangeError);
  assert.throws(() => call(ok, new Float64Array([0])), RangeError);
  m.dispose();
  console.log('beats_gpu: 4 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
