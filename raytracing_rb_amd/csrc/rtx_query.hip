// rtx_query.hip — batched World#lit_area / World#local_lights (DESIGN.md
// "Batched World queries"): for n explicit targets,
//
//   World#lit_area(target, light.position, light.radius)   (src/world.rb:62-69)
//   World#local_lights(position)                            (src/world.rb:72-80)
//
// against every light of the scene in order, or against one explicit
// {position, radius} per target:
//
//   area[i][k]  = max(1 - ordered sum of the cover areas, 0)
//   color[i][k] = light_k.color * (area ** soft_shadow_exponent / n_lights), zeros where area == 0
//   status[i]   = rtx_status of the first raise of target i in light order (cover_area's Math.acos,
//                 sphere.rb:45-46), else 0; the raising light's entries and all later ones are NaN
//
// One target per lane, consecutive targets in consecutive lanes.  The walk of
// each (target, light) is the lanes engine's SHADOW query (rtx_kernels.hip
// k_render, state B/C): the ordered linear walk, or the hierarchy walk with
// per-lane traversal stacks and cover lists in LDS, which repeats the ordered
// walk where more than COVER_K covers are non-zero.  The colour is the first
// half of light_term (rtx_device.h).  Binary64 in the reference's operation
// order (-ffp-contract=off): a query answers what a render would use.
#include "rtx_device.h"

namespace rtx {

constexpr int LA_BS = 256;

// device ERR_ code (rtx_vec3.h) -> rtx_status, as report_errors (rtx_capi.cpp)
__device__ __forceinline__ int32_t la_status(uint32_t code) { return code == ERR_TYPE ? 8 : (int32_t)code; }

// SPH: SPH_LIN_SCALAR, SPH_BVH_LDS (hierarchy nodes and leaf records staged in
// LDS) or SPH_BVH_GLOBAL.  lights: null (the scene's lights) or 4 doubles per
// target.  color, status: may be null.
template <int SPH>
__global__ __launch_bounds__(LA_BS) void k_lit_area(KParams p, const double* __restrict__ targets,
                                                     const double* __restrict__ lights, double* __restrict__ area,
                                                     double* __restrict__ color, int32_t* __restrict__ status) {
  const SceneDev& S = p.scene;                  // kernel argument: scalar loads
  extern __shared__ float4 lds_la[];
  char* lds = reinterpret_cast<char*>(lds_la);
  if (SPH == SPH_BVH_LDS) {
    const int nn = S.n_nodes * (int)(sizeof(Bvh4Node) / 16);
    for (int i = threadIdx.x; i < nn; i += LA_BS) lds_la[i] = reinterpret_cast<const float4*>(S.bvh)[i];
    float4* leaf = reinterpret_cast<float4*>(lds + p.lds_leaf);
    for (int i = threadIdx.x; i < S.n_slots; i += LA_BS) leaf[i] = reinterpret_cast<const float4*>(S.bvh_sph32)[i];
    __syncthreads();                            // (the only barrier)
  }
  // A lane past the batch leaves before any walk: the hierarchy walk ballots over the lanes that entered it.
  const size_t i = (size_t)blockIdx.x * LA_BS + threadIdx.x;
  if (i >= (size_t)p.nrays) return;
  int* stk = reinterpret_cast<int*>(lds + p.lds_stack) + threadIdx.x;
  int* cov_i = reinterpret_cast<int*>(lds + p.lds_cov) + threadIdx.x;
  double* cov_v = reinterpret_cast<double*>(lds + p.lds_cov + COVER_K * LA_BS * 4) + threadIdx.x;

  const V3 T = v3p(targets + 3 * i);
  const int nl = lights ? 1 : S.n_light;
  const bool xr = p.exact_raises != 0;          // the walk also checks its covers' acos raises (rtx_device.h xr_band)
  const double nan = __builtin_nan("");
  uint32_t err = 0;                             // this target's first raise
  int32_t st = 0;
  for (int k = 0; k < nl; k++) {
    V3 L, lcol = v3(0.0, 0.0, 0.0);
    double rad;
    if (lights) {
      L = v3p(lights + 4 * i);
      rad = lights[4 * i + 3];
    } else {
      const LightDev& LD = S.light[k];
      L = v3p(LD.pos);
      rad = LD.radius;
      lcol = v3p(LD.color);
    }
    double a = nan;
    V3 c = v3(nan, nan, nan);
    if (!st) {                                  // (after a raise the reference computes nothing more)
      const V3 d = vsub(L, T);                  // Ray(light - target, target)
      double best = S.max_distance, total = 1.0;
      int besti = -1;
      bool hin = true;
      V3 hit = v3(0.0, 0.0, 0.0);
      if (SPH == SPH_LIN_SCALAR) {
        query<false>(S, cptr(S.sph32), false, T, d, L, rad, best, besti, hit, hin, total, err, nullptr, xr);
      } else {
        int q_ref = BVH_NONE, q_sp = 0, q_ncov = 0;
        bool q_ovf = false;
        if (SPH == SPH_BVH_LDS)
          query_bvh<LA_BS, false>(S, reinterpret_cast<const Bvh4Node*>(lds),
                                  reinterpret_cast<const float4*>(lds + p.lds_leaf), S.bvh_sph64, S.bvh_obj, stk,
                                  cov_i, cov_v, false, T, d, L, rad, best, besti, hit, hin, total, err, q_ref, q_sp,
                                  q_ncov, q_ovf, false, 0, xr);
        else
          query_bvh<LA_BS, false>(S, S.bvh, reinterpret_cast<const float4*>(S.bvh_sph32), S.bvh_sph64, S.bvh_obj,
                                  stk, cov_i, cov_v, false, T, d, L, rad, best, besti, hit, hin, total, err, q_ref,
                                  q_sp, q_ncov, q_ovf, false, 0, xr);
      }
      if (err & 0xffu) {
        st = la_status(err & 0xffu);
      } else {                                  // light_term's first half
        a = total > 0 ? total : 0.0;
        c = v3(0.0, 0.0, 0.0);
        if (a > 0 && color) {
          const double pw = S.sse_is_two ? a * a : rx_pow(a, S.sse);
          c = vsc(lcol, light_share(S, pw));
        }
      }
    }
    const size_t o = i * (size_t)nl + (size_t)k;
    area[o] = a;
    if (color) {
      color[3 * o] = c.x;
      color[3 * o + 1] = c.y;
      color[3 * o + 2] = c.z;
    }
  }
  if (status) status[i] = st;
}

template <int SPH>
static hipError_t launch_la(const KParams& p, size_t lds, const double* d_targets, const double* d_lights,
                            double* d_area, double* d_color, int32_t* d_status, hipStream_t s) {
  if (lds > 64 * 1024) {                        // deep traversal stacks: raise the kernel's dynamic-LDS limit once
    int cus, per_cu;
    const hipError_t e = launch_fit(reinterpret_cast<const void*>(k_lit_area<SPH>), LA_BS, lds, cus, per_cu);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)(((size_t)p.nrays + LA_BS - 1) / LA_BS));
  hipLaunchKernelGGL(k_lit_area<SPH>, grid, dim3(LA_BS), lds, s, p, d_targets, d_lights, d_area, d_color, d_status);
  return hipGetLastError();
}

// Workgroups per CU the kernel's registers allow (161 VGPRs: 3 waves per SIMD): the hierarchy is
// staged only while its LDS image leaves that occupancy (as FH_WGS_PER_CU, rtx_aov.hip).
constexpr int LA_WGS_PER_CU = 3;

// mode: the context's SphMode.  A linear mode walks the ordered scan; every
// hierarchy mode walks the four-wide hierarchy in SHADOW mode.  LDS holds the
// per-lane traversal stacks (bvh_stack x LA_BS x 4 bytes), the cover lists
// (COVER_K x LA_BS x 12 bytes: int32 object indices, then binary64 areas) and,
// in front of them, the hierarchy's nodes and leaf records when the hierarchy
// workgroup's layout holds them (resolve_mode, bvh_lds_bytes) and this
// kernel's image fits LA_WGS_PER_CU times per CU; otherwise (C4) they are read
// from global memory.
hipError_t launch_lit_area(KParams p, int mode, const double* d_targets, const double* d_lights, double* d_area,
                           double* d_color, int32_t* d_status, hipStream_t s) {
  if (p.nrays <= 0) return hipSuccess;
  const SceneDev& S = p.scene;
  if (!sph_is_bvh(mode) || S.bvh_root == BVH_NONE)
    return launch_la<SPH_LIN_SCALAR>(p, 0, d_targets, d_lights, d_area, d_color, d_status, s);
  const size_t stacks = (((size_t)S.bvh_stack * LA_BS * 4) + 15) & ~(size_t)15;
  const size_t covers = (size_t)COVER_K * LA_BS * 12;
  const size_t records = ((size_t)S.n_nodes * sizeof(Bvh4Node) + (size_t)S.n_slots * 16 + 15) & ~(size_t)15;
  const bool staged = mode != SPH_BVH_GLOBAL && resolve_mode(S, SPH_BVH_LDS) == SPH_BVH_LDS &&
                      records + stacks + covers <= LDS_TOTAL_BYTES / LA_WGS_PER_CU;
  size_t off = 0;
  if (staged) {
    p.lds_leaf = (int32_t)((size_t)S.n_nodes * sizeof(Bvh4Node));
    off = records;
  }
  p.lds_stack = (int32_t)off;
  off += stacks;
  p.lds_cov = (int32_t)off;
  off += covers;
  if (off > LDS_TOTAL_BYTES) return hipErrorInvalidValue;
  return staged ? launch_la<SPH_BVH_LDS>(p, off, d_targets, d_lights, d_area, d_color, d_status, s)
                : launch_la<SPH_BVH_GLOBAL>(p, off, d_targets, d_lights, d_area, d_color, d_status, s);
}

}  // namespace rtx
