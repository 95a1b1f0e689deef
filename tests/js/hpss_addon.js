'use strict';
// A stand-in for meyda_napi.node that records every call (host-side tests of the facade's HPSS plumbing only,
// tests/js/hpss_facade.js; never used by the product): the plan calls the facade makes, chromaWeights,
// which returns an array of the stated size, and hpssGather, which returns arrays of the stated sizes for what its
// options ask for.
const calls = [];
function gather(fn) {
  return (plan, samples, starts, frameOffsets, o) => {
    calls.push({ fn, args: [samples, starts, frameOffsets, o] });
    const F = starts.length, S = frameOffsets.length - 1, cols = 128, r = {};
    if (o.harmonic) r.harmonic = new Float32Array(F * cols).fill(1);
    if (o.percussive) r.percussive = new Float32Array(F * cols).fill(2);
    if (o.chroma) {
      r.numChroma = o.chroma.numChroma;
      if (o.chroma.perFrame) r.chroma = new Float32Array(F * o.chroma.numChroma).fill(3);
      if (o.chroma.summary) r.chromaSummary = Float64Array.from({ length: S * 4 * o.chroma.numChroma }, (_, i) => i);
    }
    if (o.flux) {
      if (o.flux.perFrame) r.flux = new Float32Array(F).fill(4);
      if (o.flux.summary) r.fluxSummary = Float64Array.from({ length: S * 4 }, (_, i) => i);
    }
    return fn === 'hpssGatherAsync' ? Promise.resolve(r) : r;
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
  chromaWeights: (n, sr, o) => {
    calls.push({ fn: 'chromaWeights', args: [n, sr, o] });
    return new Float32Array(o.numChroma * n / 2).fill(0.5);
  },
  hpssGather: gather('hpssGather'),
  hpssGatherAsync: gather('hpssGatherAsync'),
};
