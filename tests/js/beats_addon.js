'use strict';
// A stand-in for meyda_napi.node that records every call (host-side tests of the facade's beat plumbing only,
// tests/js/beats_facade.js; never used by the product): the tempo stand-in (tests/js/tempo_addon.js) with beatTables,
// which returns arrays of the stated sizes that name their arguments, and beatsGather, which returns the lags of the
// tempo stand-in and for signal s the beats at its first buffer + 1 and + 2 (none for a signal without two buffers).
const tempo = require('./tempo_addon');
const calls = tempo.calls;
function gather(fn) {
  return (plan, samples, starts, frameOffsets, o) => {
    const r = tempo.tempoGather(plan, samples, starts, frameOffsets, o);
    calls[calls.length - 1].fn = fn;
    const S = frameOffsets.length - 1, rows = [], off = [0];
    for (let s = 0; s < S; ++s) {
      if (frameOffsets[s + 1] - frameOffsets[s] > 2) rows.push(frameOffsets[s] + 1, frameOffsets[s] + 2);
      off.push(rows.length);
    }
    r.beatOffsets = Float64Array.from(off);
    r.beats = Float64Array.from(rows);
    return fn === 'beatsGatherAsync' ? Promise.resolve(r) : r;
  };
}
module.exports = Object.assign({}, tempo, {
  beatTables: (P, tightness) => {
    calls.push({ fn: 'beatTables', args: [P, tightness] });
    return { gauss: new Float32Array((P + 1) * (P + 2) / 2).fill(P), penalty: new Float64Array((P + 1) * (P + 1)).fill(tightness) };
  },
  beatsGather: gather('beatsGather'),
  beatsGatherAsync: gather('beatsGatherAsync'),
});
