'use strict';
// A stand-in for meyda_napi.node that records every call (host-side tests of the facade's tempo plumbing only,
// tests/js/tempo_facade.js; never used by the product): tempoGather returns the lags 0, 86, 43, ... and a summary
// whose values tell the signal, the statistic and the lag; the window and the prior are arrays of the asked length
// that name their arguments.
const calls = [];
const LAGS = [0, 86, 43, 7];
function gather(fn) {
  return (plan, samples, starts, frameOffsets, o) => {
    calls.push({ fn, args: [samples, starts, frameOffsets, o] });
    const S = frameOffsets.length - 1, L = o.numLags;
    const r = { lag: new Uint32Array(S), numLags: L };
    for (let s = 0; s < S; ++s) r.lag[s] = LAGS[s % LAGS.length];
    if (o.mean) {
      r.summary = new Float64Array(S * 4 * L);
      for (let s = 0; s < S; ++s) for (let j = 0; j < 4; ++j) for (let l = 0; l < L; ++l) r.summary[(s * 4 + j) * L + l] = 1000 * s + 100 * j + l;
    }
    if (o.envelope) r.envelope = new Float32Array(starts.length);
    return fn === 'tempoGatherAsync' ? Promise.resolve(r) : r;
  };
}
module.exports = {
  calls,
  hostTables: ({ bufferSize }) => ({ barkScale: new Float32Array(bufferSize), hanning: new Float32Array(bufferSize),
    hamming: new Float32Array(bufferSize) }),
  createPlan: (o) => ({ o }),
  destroyPlan: () => {},
  planBusy: () => false,
  isPowerOfTwo: (v) => v > 0 && (v & (v - 1)) === 0,
  signalsFrameStarts: (lengths, N, H) => {
    const fo = [0], st = [];
    let at = 0;
    for (const S of lengths) {
      const F = S < N ? 0 : Math.floor((S - N) / H) + 1;
      for (let f = 0; f < F; ++f) st.push(at + f * H);
      fo.push(st.length);
      at += S;
    }
    return { starts: Float64Array.from(st), frameOffsets: Float64Array.from(fo) };
  },
  tempogramWindow: (W) => { calls.push({ fn: 'tempogramWindow', args: [W] }); return new Float32Array(W).fill(W); },
  tempoPrior: (rate, L, o) => { calls.push({ fn: 'tempoPrior', args: [rate, L, o] }); return new Float64Array(L).fill(rate); },
  tempoGather: gather('tempoGather'),
  tempoGatherAsync: gather('tempoGatherAsync'),
};
