'use strict';
// GPU check of getSignalSummaries / getSignalSummariesAsync through the facade and the N-API addon: three
// signals pooled per signal, the shapes, the async form against the synchronous one bit for bit. Every
// statistic is written to OUT_DIR as a raw float64 file (NAME.STAT.f64), which tests/test_js_summary.py
// compares with Plan.summarize_signals. Needs an MI355X.
// usage: node summary_gpu.js SIGNAL.f32 OUT_DIR
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const [sigPath, outDir] = process.argv.slice(2);
const N = 1024, H = 256, NM = 40;
const FEATS = ['rms', 'spectralRolloff', 'mfcc', 'melBands', 'loudness', 'powerSpectrum'];
const WIDTH = { rms: 1, spectralRolloff: 1, mfcc: 13, melBands: NM, 'loudness.specific': 24, 'loudness.total': 1, powerSpectrum: N / 2 };
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

(async () => {
  const raw = fs.readFileSync(sigPath);
  const x = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.byteLength));
  // three signals: a few buffers and a partial tail, fewer samples than one buffer, exactly two buffers at this hop
  const cuts = [0, 5 * N + 77, 5 * N + 77 + N - 1, 5 * N + 77 + N - 1 + N + H];
  assert.ok(x.length >= cuts[3]);
  const signals = [0, 1, 2].map((s) => x.slice(cuts[s], cuts[s + 1]));
  const m = new Meyda({ sampleRate: 44100 }, null, N, null, { numMelBands: NM });
  const r = m.getSignalSummaries(FEATS, signals, H);
  assert.ok(r.frameOffsets instanceof Float64Array);
  assert.deepStrictEqual(Array.from(r.frameOffsets), [0, 17, 17, 19]);
  assert.deepStrictEqual(Object.keys(r).sort(), FEATS.concat(['frameOffsets']).sort());
  const f = flat(r);
  for (const k of Object.keys(f)) {
    assert.deepStrictEqual(Object.keys(f[k]), STATS, k);
    for (const st of STATS) {
      const a = f[k][st];
      assert.ok(a instanceof Float64Array && a.length === 3 * WIDTH[k], k + '.' + st);
      // the signal without buffers is NaN; the others are not
      for (let c = 0; c < WIDTH[k]; c++) {
        assert.ok(Number.isNaN(a[WIDTH[k] + c]) && !Number.isNaN(a[c]) && !Number.isNaN(a[2 * WIDTH[k] + c]), k + '.' + st);
      }
      fs.writeFileSync(path.join(outDir, k + '.' + st + '.f64'), Buffer.from(a.buffer, a.byteOffset, a.byteLength));
    }
  }
  console.log('ok getSignalSummaries: shapes, frameOffsets, the empty signal');

  const ra = await m.getSignalSummariesAsync(FEATS, signals, H);
  assert.deepStrictEqual(Array.from(ra.frameOffsets), Array.from(r.frameOffsets));
  const fa = flat(ra);
  for (const k of Object.keys(f)) {
    for (const st of STATS) {
      assert.strictEqual(fa[k][st].length, f[k][st].length);
      for (let i = 0; i < f[k][st].length; i++) assert.ok(Object.is(fa[k][st][i], f[k][st][i]), k + '.' + st + '[' + i + ']');
    }
  }
  console.log('ok the async form agrees');
  assert.strictEqual(m.getSignalSummaries('rms', [], H).rms.mean.length, 0);
  m.dispose();
  console.log('summary_gpu: 2 checks passed');
})().catch((e) => { console.error(e); process.exit(1); });
