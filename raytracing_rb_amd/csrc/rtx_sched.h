// rtx_sched.h — the chunk schedule of a bounce-level launch,
// the part the host and the device share (rtx_launch.h includes it; plain
// C++ so that tools/sched_check.cpp compiles it with g++).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTX_SCHED_HD __host__ __device__ __forceinline__
#else
#define RTX_SCHED_HD inline
#endif

namespace rtx {

constexpr int LV_ROUND_MAX = 4096;              // option lv_round: chunks a workgroup owns per round, at most

// The static part of a launch's chunks: the first S of them (option lv_static, %).
RTX_SCHED_HD uint32_t lv_static_chunks(uint32_t chunks, uint32_t pct) {
  return (uint32_t)(((uint64_t)chunks * pct) / 100);
}

// Rounds (option lv_round = R > 0): the static part is cut into rounds of R
// chunks per workgroup; workgroup b of G owns, in round k, the chunks
// k G R + b R + r, r < R.  The n-th claim of workgroup b (n counted by one
// LDS word per workgroup, whichever wave asks) is the chunk returned here:
// strictly increasing in n, so the first one >= S ends the workgroup's static
// part.  (32 bits do: a workgroup draws at most its waves' number of chunks
// past S, and S + G R + R stays far below 2^32 for R <= LV_ROUND_MAX and the
// persistent grids' G.)
RTX_SCHED_HD uint32_t lv_round_chunk(uint32_t n, uint32_t b, uint32_t G, uint32_t R) {
  const uint32_t k = n / R;
  return (k * G + b) * R + (n - k * R);
}

}  // namespace rtx
