'use strict';
// Host-side check of Meyda.beatTables through the built addon (no GPU needed) against the values tests/beat_ref.py
// computed in the same test run (tests/test_js_beats.py writes them to CASES.json: {tables: [{maxPeriod, tightness,
// gaussBits, penalty}]}, -Infinity as null): the float32 bit patterns of gauss, penalty within a relative 4 x 2^-52
// with -Infinity in the same places, and the addon's own refusals.
// usage: node beats_cpu.js CASES.json
const assert = require('assert');
const fs = require('fs');
const path = require('path');
const Meyda = require(path.join(__dirname, '..', '..', 'meyda_amd', 'js', 'meyda.js'));

const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
let n = 0;
function check(name, fn) { fn(); n++; console.log('ok ' + name); }

check('the tables agree with the numpy statement', () => {
  assert.ok(cases.tables.length >= 3);
  for (const c of cases.tables) {
    const t = c.tightness === null ? Meyda.beatTables(c.maxPeriod) : Meyda.beatTables(c.maxPeriod, c.tightness);
    const P = c.maxPeriod;
    assert.ok(t.gauss instanceof Float32Array && t.gauss.length === (P + 1) * (P + 2) / 2);
    assert.ok(t.penalty instanceof Float64Array && t.penalty.length === (P + 1) * (P + 1));
    assert.deepStrictEqual(Array.from(new Uint32Array(t.gauss.buffer, t.gauss.byteOffset, t.gauss.length)), c.gaussBits, 'gauss of ' + P);
    for (let i = 0; i < t.penalty.length; ++i) {
      if (c.penalty[i] === null) assert.strictEqual(t.penalty[i], -Infinity, 'entry ' + i + ' of ' + P);
      else assert.ok(Math.abs(t.penalty[i] - c.penalty[i]) <= 4 * Math.pow(2, -52) * Math.abs(c.penalty[i]), 'entry ' + i + ' of ' + P);
    }
  }
});

check('the addon\'s own refusals', () => {
  assert.throws(() => Meyda.addon.beatTables(0), RangeError);
  assert.throws(() => Meyda.addon.beatTables(1024), RangeError);
  assert.throws(() => Meyda.addon.beatTables('8'), TypeError);
  assert.throws(() => Meyda.addon.beatTables(8, '100'), TypeError);
  assert.throws(() => Meyda.addon.beatTables(8, -1), Error);
  assert.throws(() => Meyda.addon.beatTables(8, NaN), Error);
  assert.throws(() => Meyda.addon.beatsGather(), TypeError);
});

console.log('beats_cpu: ' + n + ' checks passed');
