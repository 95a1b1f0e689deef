'use strict';
// A stand-in for meyda_napi.node that records every call (host-side tests of the facade's hopSize
// plumbing only, tests/js/facade_signal.js; never used by the product): which addon function ran and with
// which arguments, nothing computed.
const calls = [];
const rec = (fn, ret) => (...args) => { calls.push({ fn, args }); return ret === undefined ? {} : ret(...args); };
module.exports = {
  calls,
  hostTables: ({ bufferSize }) => ({ barkScale: new Float32Array(bufferSize), hanning: new Float32Array(bufferSize),
    hamming: new Float32Array(bufferSize) }),
  createPlan: (o) => ({ o }),
  destroyPlan: () => {},
  planBusy: () => false,
  extract: rec('extract'),
  extractAsync: rec('extractAsync', () => Promise.resolve({})),
  extractWav: rec('extractWav'),
  extractWavAsync: rec('extractWavAsync', () => Promise.resolve({})),
  extractSignal: rec('extractSignal'),
  extractSignalAsync: rec('extractSignalAsync', () => Promise.resolve({})),
  signalFrames: rec('signalFrames', (S, N, H) => (S < N ? 0 : Math.floor((S - N) / H) + 1)),
};
