'use strict';
// GPU check of getSignalSummaries / getSignalSummariesAsync with {deltaWidth, deltaOrder} through the facade and
// the N-API addon: three signals pooled per signal, `delta` and `delta2` of the base result's shape, every value
// against the Python binding's (Plan.summarize_signals with deltas, written by tests/test_js_delta.py to DIR as
// raw float64 files ORDER.NAME.STAT.f64, ORDER being base, delta or delta2), the async form against the
// synchronous one bit for bit, and the result without the option against the call that has none. Needs an MI355X.
// usage: node delta_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 1024, H = 256, NM = 40;
const FEATS = ['rms', 'spectralRolloff', 'mfcc', 'melBands', 'loudness'];
const WIDTH = { rms: 1, spectralRolloff: 1, mfcc: 13, melBands: NM, 'loudness.specific': 24, 'loudness.total': 1 };
const STATS = ['mean', 'variance', 'min', 'max'];
process.on('unhandledRejection', (e) => { console.error(e); process.exit(1); });

function flat(r) {
  const o = {};
  for (const k of FEATS) {
    if (k === 'loudness') {
      o['loudness.specific'] = r.loudness.specific;
      o['loudness.total'] = r.loudness.total;
    } else {
      o[k] = r[k];
    }
  }
  return o;
}

function sameBits(a, b, what) {
  assert.ok(a instanceof Float64Array && b instanceof Float64Array && a.length === b.length, what);
  const x = new BigUint64Array(a.buffer, a.byteOffset, a.length), y = new BigUint64Array(b.buffer, b.byteOffset, b.length);
  for (let i = 0; i < x.length; i++) assert.ok(x[i] === y[i], what + '[' + i + ']: ' + a[i] + ' against ' + b[i]);
}

function expected(order, k, st) {
  const raw = fs.readFileSync(path.join(dir, order + '.' + k + '.' + st + '.f64'));
  return new Float64Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
}

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  // three signals: a few buffers and a partial tail, fewer samples than one buffer, exactly two buffers at this hop
  const cuts = [0, 5 * N + 77, 5 * N + 77 + N - 1, 5 * N + 77 + N - 1 + N + H];
  assert.ok(x.length >= cuts[3]);
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: 44100 }, null, N, null, { numMelBands: NM });
  const r = m.getSignalSummaries(FEATS, signals, H, { deltaWidth: 2, deltaOrder: 2 });
  assert.deepStrictEqual(Object.keys(r).sort(), FEATS.concat(['frameOffsets', 'delta', 'delta2']).sort());
  const orders = { base: r, delta: r.delta, delta2: r.delta2 };
  for (const order of Object.keys(orders)) {
    const o = orders[order];
    assert.deepStrictEqual(Array.from(o.frameOffsets), [0, 17, 17, 19], order);
    assert.deepStrictEqual(Object.keys(o).filter((k) => k !== 'delta' && k !== 'delta2').sort(), FEATS.concat(['frameOffsets']).sort(), order);
    const f = flat(o);
    for (const k of Object.keys(f)) {
      assert.deepStrictEqual(Object.keys(f[k]), STATS, order + '.' + k);
      for (const st of STATS) {
        const a = f[k][st];
        assert.ok(a instanceof Float64Array && a.length === 3 * WIDTH[k], order + '.' + k + '.' + st);
        // the signal without buffers is NaN; the others are not
        for (let c = 0; c < WIDTH[k]; c++) {
          assert.ok(Number.isNaN(a[WIDTH[k] + c]) && !Number.isNaN(a[c]) && !Number.isNaN(a[2 * WIDTH[k] + c]), order + '.' + k + '.' + st);
        }
        sameBits(a, expected(order, k, st), order + '.' + k + '.' + st);
      }
    }
  }
  console.log('ok delta and delta2: the shapes, the empty signal, the Python binding\'s values');

  const ra = await m.getSignalSummariesAsync(FEATS, signals, H, { deltaWidth: 2, deltaOrder: 2 });
  const oa = { base: ra, delta: ra.delta, delta2: ra.delta2 };
  for (const order of Object.keys(orders)) {
    const f = flat(orders[order]), fa = flat(oa[order]);
    for (const k of Object.keys(f)) for (const st of STATS) sameBits(fa[k][st], f[k][st], 'async ' + order + '.' + k + '.' + st);
  }
  console.log('ok the async form agrees');

  // order 1 has no delta2, and its delta is the one of order 2; the defaults are width 2, order 2
  const r1 = m.getSignalSummaries(FEATS, signals, H, { deltaOrder: 1 });
  assert.ok(r1.delta && !('delta2' in r1));
  for (const st of STATS) sameBits(r1.delta.mfcc[st], r.delta.mfcc[st], 'order 1 mfcc.' + st);
  const rd = m.getSignalSummaries(['mfcc'], signals, H, { deltaWidth: 2 });
  for (const st of STATS) sameBits(rd.delta2.mfcc[st], r.delta2.mfcc[st], 'default order mfcc.' + st);
  // without the option, and with options that name no delta, the result is the existing call's
  const plain = m.getSignalSummaries(FEATS, signals, H);
  assert.ok(!('delta' in plain) && !('delta2' in plain));
  assert.deepStrictEqual(m.getSignalSummaries(FEATS, signals, H, {}), plain);
  assert.deepStrictEqual(m.getSignalSummaries(FEATS, signals, H, undefined), plain);
  assert.deepStrictEqual(await m.getSignalSummariesAsync(FEATS, signals, H, null), plain);
  for (const k of Object.keys(flat(plain))) for (const st of STATS) sameBits(flat(plain)[k][st], flat(r)[k][st], 'base beside deltas ' + k + '.' + st);
  console.log('ok without the option the result is unchanged');

  // the deltas of a spectrum are not pooled: the library's message; bad options are refused by the facade
  for (const bad of ['powerSpectrum', ['rms', 'amplitudeSpectrum']]) {
    assert.throws(() => m.getSignalSummaries(bad, signals, H, { deltaOrder: 2 }), /deltas of a spectrum are not pooled/);
    await assert.rejects(m.getSignalSummariesAsync(bad, signals, H, { deltaOrder: 1 }), /deltas of a spectrum are not pooled/);
  }
  for (const w of [0, 9, 1.5, '2']) assert.throws(() => m.getSignalSummaries('rms', signals, H, { deltaWidth: w }), RangeError);
  for (const o of [0, 3, '1']) assert.throws(() => m.getSignalSummaries('rms', signals, H, { deltaOrder: o }), RangeError);
  assert.throws(() => m.getSignalSummaries('rms', signals, H, 2), TypeError);
  assert.strictEqual(m.getSignalSummaries('rms', [], H, { deltaOrder: 2 }).delta2.rms.mean.length, 0);
  m.dispose();
  console.log('delta_gpu: 4 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
