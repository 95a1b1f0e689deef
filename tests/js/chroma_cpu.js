'use strict';
// Host-side check of Meyda.chromaFilterBank (no GPU needed): the bank through the built addon against the values
// tests/chroma_ref.py computed in the same test run (tests/test_js_chroma.py writes them to CASES.json: a list of
// {bufferSize, sampleRate, options, bits}, bits the float32 table's uint32 patterns), within one unit of the last
// place per entry, and the refusals.
// usage: node chroma_cpu.js CASES.json
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
let n = 0;
function check(name, fn) { fn(); n++; console.log('ok ' + name); }

check('the bank agrees with the numpy statement', () => {
  assert.ok(cases.length >= 8);
  for (const c of cases) {
    const w = Meyda.chromaFilterBank(c.bufferSize, c.sampleRate, c.options);
    const C = c.options && c.options.numChroma !== undefined ? c.options.numChroma : 12;
    assert.ok(w instanceof Float32Array && w.length === C * c.bufferSize / 2 && w.length === c.bits.length, JSON.stringify(c.options));
    const u = new Uint32Array(w.buffer, w.byteOffset, w.length);
    for (let i = 0; i < u.length; ++i) {
      // (positive floats: their bit patterns are ordered as they are)
      assert.ok(Math.abs(u[i] - c.bits[i]) <= 1, 'entry ' + i + ' of ' + JSON.stringify([c.bufferSize, c.sampleRate, c.options]));
      assert.ok(Number.isFinite(w[i]) && w[i] > 0);
    }
  }
});

check('the defaults', () => {
  const a = Meyda.chromaFilterBank(1024, 44100);
  const b = Meyda.chromaFilterBank(1024, 44100, { numChroma: 12, a440: 440, centerOctave: 5, octaveWidth: 2, baseC: true });
  assert.deepStrictEqual(Array.from(a), Array.from(b));
  assert.strictEqual(a.length, 12 * 512);
  const c = Meyda.chromaFilterBank(1024, 44100, { baseC: false });
  // row 0 is A without baseC: it is row 9 of the table whose row 0 is C
  assert.deepStrictEqual(Array.from(c.subarray(0, 512)), Array.from(a.subarray(9 * 512, 10 * 512)));
  assert.strictEqual(Meyda.addon.chromaWeights(1024, 44100).length, 12 * 512);
});

check('the refusals', () => {
  for (const nbuf of [0, 2, 3, 1000, 1025, '1024', undefined]) assert.throws(() => Meyda.chromaFilterBank(nbuf, 44100), Error);
  for (const sr of [0, -1, Infinity, NaN, '44100']) assert.throws(() => Meyda.chromaFilterBank(1024, sr), RangeError);
  const bad = (o, E) => assert.throws(() => Meyda.chromaFilterBank(1024, 44100, o), E);
  bad(3, TypeError);
  for (const numChroma of [0, 37, 1.5, '12']) bad({ numChroma }, RangeError);
  for (const a440 of [0, -440, Infinity, NaN, '440']) bad({ a440 }, RangeError);
  for (const octaveWidth of [-1, Infinity, NaN]) bad({ octaveWidth }, RangeError);
  for (const centerOctave of [Infinity, NaN, '5']) bad({ centerOctave }, RangeError);
  assert.strictEqual(Meyda.chromaFilterBank(4, 44100, { numChroma: 1, octaveWidth: 0 }).length, 2);
  // the addon's own checks, past the facade's
  assert.throws(() => Meyda.addon.chromaWeights(1000, 44100), Error);
  assert.throws(() => Meyda.addon.chromaWeights(1024, 44100, { numChroma: 37 }), RangeError);
  assert.throws(() => Meyda.addon.chromaWeights(1024, 0), Error);
  assert.throws(() => Meyda.addon.chromaWeights('1024', 44100), TypeError);
});

console.log('chroma_cpu: ' + n + ' checks passed');
