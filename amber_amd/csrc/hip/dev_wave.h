// dev_wave.h -- part of pt_device.h (included from there, first; not a stand-alone header): what the lanes of a wave settle among themselves -- a lane's
// rank in a ballot, and the hand-out of indices from a block the wave claimed with one atomic.
#pragma once

namespace amber_dev {

// The number of set bits of `mask` below this lane: its rank among the lanes that voted (the mask of a __ballot).
__device__ __forceinline__ uint32_t WaveRank(unsigned long long mask) {
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

// A wave's open block [next, end) of the indices 0 .. n - 1 that persistent waves claim from one counter, kClaim at a time.  Wave-uniform (SGPRs).
struct WaveClaim {
  uint32_t next = 0, end = 0;
  bool exhausted = false;                  // the counter has passed n: nothing is left to claim
};

// Every lane that wants an index takes the next one of the wave's block, in lane order; an empty block is replaced by the next kClaim indices of
// `counter` (one atomicAdd by lane 0; n <= 2^31 and every wave adds once more at most: no wrap).  Returns whether this lane got one, in `index`;
// a lane goes without only when the counter is exhausted.  Call with the wave's lanes converged.
template <uint32_t kClaim>
__device__ __forceinline__ bool ServeLanes(WaveClaim& claim, unsigned int* counter, uint32_t n, uint32_t lane, bool want, uint32_t& index) {
  bool got = false;
  unsigned long long mw = __ballot(want);
  while (mw != 0ull) {
    const uint32_t avail = claim.end - claim.next;
    if (avail == 0u) {
      if (claim.exhausted) break;
      uint32_t base = 0;
      if (lane == 0u) base = atomicAdd(counter, kClaim);
      base = __builtin_amdgcn_readfirstlane(base);
      if (base >= n) { claim.exhausted = true; break; }
      claim.next = base; claim.end = n - base < kClaim ? n : base + kClaim;
      continue;
    }
    const uint32_t rank = WaveRank(mw);
    if (want && rank < avail) { index = claim.next + rank; want = false; got = true; }
    const uint32_t wanted = static_cast<uint32_t>(__popcll(mw));
    claim.next += wanted < avail ? wanted : avail;
    mw = __ballot(want);
  }
  return got;
}

}  // namespace amber_dev
