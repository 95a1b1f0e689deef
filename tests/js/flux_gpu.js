'use strict';
// GPU check of getSignalSummaries / getSignalSummariesAsync with {flux: [...]} through the facade and the N-API
// addon: three signals, four flux requests; every statistic and every per-frame column against the Python
// binding's (Plan.summarize_signals with flux, written by tests/test_js_flux.py to DIR as raw files
// flux.I.STAT.f64 and flux.I.perFrame.f32), the async form against the synchronous one bit for bit, flux beside
// deltas, and the result without the option against the call that has none. Needs an MI355X.
// usage: node flux_gpu.js SIGNAL.f32 DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, dir] = process.argv.slice(2);
const N = 1024, H = 256, NM = 40;
const FEATS = ['rms', 'mfcc'];
const STATS = ['mean', 'variance', 'min', 'max'];
// (as tests/test_js_flux.py asks for them)
const FLUX = [{ feature: 'melBands', perFrame: true }, { feature: 'amplitudeSpectrum', mode: 'l2', lag: 2, perFrame: true },
  { feature: 'mfcc', mode: 'l1', lag: 8 }, { feature: 'loudness', mode: 'rectified', lag: 1, perFrame: false }];
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

function sameFlux(a, b, what) {
  assert.strictEqual(a.length, b.length, what);
  a.forEach((f, i) => {
    assert.deepStrictEqual(Object.keys(f), Object.keys(b[i]), what + ' ' + i);
    for (const k of Object.keys(f)) sameBits(f[k], b[i][k], what + ' ' + i + '.' + k);
  });
}

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  // three signals: a few buffers and a partial tail, fewer samples than one buffer, exactly two buffers at this hop
  const cuts = [0, 5 * N + 77, 5 * N + 77 + N - 1, 5 * N + 77 + N - 1 + N + H];
  assert.ok(x.length >= cuts[3]);
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: 44100 }, null, N, null, { numMelBands: NM });
  const r = m.getSignalSummaries(FEATS, signals, H, { flux: FLUX });
  // flux and no delta key: no deltas
  assert.deepStrictEqual(Object.keys(r).sort(), FEATS.concat(['frameOffsets', 'flux']).sort());
  assert.deepStrictEqual(Array.from(r.frameOffsets), [0, 17, 17, 19]);
  assert.strictEqual(r.flux.length, FLUX.length);
  r.flux.forEach((f, i) => {
    assert.deepStrictEqual(Object.keys(f), FLUX[i].perFrame ? STATS.concat(['perFrame']) : STATS, 'flux ' + i);
    for (const st of STATS) {
      assert.ok(f[st] instanceof Float64Array && f[st].length === 3, 'flux ' + i + '.' + st);
      // the signal without buffers is NaN; the others are not
      assert.ok(Number.isNaN(f[st][1]) && !Number.isNaN(f[st][0]) && !Number.isNaN(f[st][2]), 'flux ' + i + '.' + st);
      sameBits(f[st], expected('flux.' + i + '.' + st + '.f64', Float64Array), 'flux ' + i + '.' + st);
    }
    if (FLUX[i].perFrame) {
      assert.ok(f.perFrame instanceof Float32Array && f.perFrame.length === 19, 'flux ' + i + '.perFrame');
      assert.ok(f.perFrame[0] === 0 && f.perFrame[17] === 0 && f.perFrame[1] > 0 && f.perFrame[18] > 0, 'flux ' + i + ' first rows');
      sameBits(f.perFrame, expected('flux.' + i + '.perFrame.f32', Float32Array), 'flux ' + i + '.perFrame');
    }
  });
  console.log('ok flux: the shapes, the empty signal, the Python binding\'s values');

  const ra = await m.getSignalSummariesAsync(FEATS, signals, H, { flux: FLUX });
  sameFlux(ra.flux, r.flux, 'async');
  for (const st of STATS) sameBits(ra.mfcc[st], r.mfcc[st], 'async mfcc.' + st);
  console.log('ok the async form agrees');

  // beside deltas: the same flux, and the deltas of the call without flux
  const rd = m.getSignalSummaries(FEATS, signals, H, { deltaOrder: 2, flux: FLUX });
  const d = m.getSignalSummaries(FEATS, signals, H, { deltaOrder: 2 });
  assert.ok(rd.delta && rd.delta2 && !('flux' in d));
  sameFlux(rd.flux, r.flux, 'beside deltas');
  for (const k of ['delta', 'delta2']) for (const st of STATS) sameBits(rd[k].mfcc[st], d[k].mfcc[st], k + '.mfcc.' + st);
  console.log('ok flux beside deltas');

  // without the option the result is the existing call's, and the base summaries beside flux are its values
  const plain = m.getSignalSummaries(FEATS, signals, H);
  assert.ok(!('flux' in plain) && !('delta' in plain));
  assert.deepStrictEqual(m.getSignalSummaries(FEATS, signals, H, {}), plain);
  for (const k of FEATS) for (const st of STATS) sameBits(plain[k][st], r[k][st], 'base beside flux ' + k + '.' + st);
  // defaults: mode 'rectified', lag 1
  const dflt = m.getSignalSummaries('rms', signals, H, { flux: [{ feature: 'loudness' }] });
  for (const st of STATS) sameBits(dflt.flux[0][st], r.flux[3][st], 'defaults ' + st);
  console.log('ok without the option the result is unchanged');

  // bad requests are refused by the facade
  const bad = (flux, E) => assert.throws(() => m.getSignalSummaries('rms', signals, H, { flux }), E);
  bad([], RangeError);
  bad([FLUX[0], FLUX[0], FLUX[0], FLUX[0], FLUX[0]], RangeError);
  bad({ feature: 'mfcc' }, RangeError);
  bad([{ feature: 'rms' }], TypeError);
  bad([{ feature: 'complexSpectrum' }], TypeError);
  bad(['mfcc'], TypeError);
  bad([{ feature: 'mfcc', mode: 'l3' }], RangeError);
  for (const lag of [0, 9, 1.5, '2']) bad([{ feature: 'mfcc', lag }], RangeError);
  assert.throws(() => m.getSignalSummaries('rms', signals, H, 2), TypeError);
  m.dispose();
  console.log('flux_gpu: 5 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
