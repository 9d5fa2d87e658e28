// rtx_rtmap.hip — batched RayTracer#rt_map and Camera#lens_func (DESIGN.md
// "Batched rt_map and lens rays"):
//
//   Camera#lens_func(x, y, sample)           (src/camera.rb:129-151)
//   RayTracer#rt_map(item), one call per item (src/ray_tracer.rb:50-164)
//
// k_lens_rays: the rays lens_func draws for the pixels of a rectangle, one
// pixel per lane, by the render's own lens_target / lens_ray.
//
// k_rt_map: for n explicit items {ray, attenuation, (x, y, sample, depth), path}
// what one rt_map call produces:
//
//   info[6]        = {status, kind, object, n_children, n_leaves, direction}
//   children[CMAX] = {front, position, item.att * att_x}, in rt_map's push order (reflection,
//                    refraction if any, the path-tracing rays), compacted; CMAX = 2 + pt
//   child_paths    = path * (pt + 3) + slot (1 reflection, 2 refraction, 3 + k path-tracing ray k)
//   leaves[LMAX]   = the colours rt_map appends, times the item's attenuation; LMAX = max(n_lights, 1)
//
//   kind 0 dead (ray_tracer.rb:52), 1 highlight (:60-77), 2 miss, 3 hit with a lit light (the
//   local-lighting leaf), 4 hit with none (pt path-tracing children), -1 a raise.
//
// One item per lane, consecutive items in consecutive lanes, in the lanes
// engine's sequence (rtx_kernels.hip k_render) built from the same device
// functions (rtx_device.h): the cutoff, the highlights with their lit_area
// raise walk, the nearest-hit walk, hit_info, one shadow walk and light_term
// per light, then shade_finish's tail writing records where the engine calls
// emit.  rt_map returns children that die on their next pop (depth 0, a tiny
// attenuation); so does this kernel: emit's drop is the engines' and every
// child is built in full.  Binary64 in the reference's operation order
// (-ffp-contract=off): a tree rebuilt level by level through this kernel and
// summed in trace_sync's order has the bits of rtx_trace.
//
// The device evaluates rt_map's raise sites in another order than the reference
// (the shadow walks before the children), so each group keeps its own error word
// and the words are merged in the reference's order (as lv_finish, rtx_levels.hip).
#include "rtx_device.h"

namespace rtx {

constexpr int RM_BS = 256;

// device ERR_ code (rtx_vec3.h) -> rtx_status, as report_errors (rtx_capi.cpp)
__device__ __forceinline__ int32_t rm_status(uint32_t code) { return code == ERR_TYPE ? 8 : (int32_t)code; }

// Three / six / nine doubles at g (8-byte aligned): pairs where the address allows.
__device__ __forceinline__ void rm_store3(double* g, V3 a) {
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    *reinterpret_cast<double2*>(g) = make_double2(a.x, a.y);
    g[2] = a.z;
  } else {
    g[0] = a.x;
    *reinterpret_cast<double2*>(g + 1) = make_double2(a.y, a.z);
  }
}
__device__ __forceinline__ void rm_store6(double* g, V3 a, V3 b) {
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    double2* g2 = reinterpret_cast<double2*>(g);
    g2[0] = make_double2(a.x, a.y);
    g2[1] = make_double2(a.z, b.x);
    g2[2] = make_double2(b.y, b.z);
  } else {
    double2* g2 = reinterpret_cast<double2*>(g + 1);
    g[0] = a.x;
    g2[0] = make_double2(a.y, a.z);
    g2[1] = make_double2(b.x, b.y);
    g[5] = b.z;
  }
}
__device__ __forceinline__ void rm_store9(double* g, V3 a, V3 b, V3 c) {
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    double2* g2 = reinterpret_cast<double2*>(g);
    g2[0] = make_double2(a.x, a.y);
    g2[1] = make_double2(a.z, b.x);
    g2[2] = make_double2(b.y, b.z);
    g2[3] = make_double2(c.x, c.y);
    g[8] = c.z;
  } else {
    double2* g2 = reinterpret_cast<double2*>(g + 1);
    g[0] = a.x;
    g2[0] = make_double2(a.y, a.z);
    g2[1] = make_double2(b.x, b.y);
    g2[2] = make_double2(b.z, c.x);
    g2[3] = make_double2(c.y, c.z);
  }
}

// Camera#lens_func for pixel idx (row-major, rows top-down as rtx_render) of the region of `p`:
// rays[idx] = {front (not normalized), position}.  A 48-byte record: three pairs in a 16-byte
// aligned buffer, the lanes of a wave writing one contiguous 3 KB run.
__global__ __launch_bounds__(RM_BS) void k_lens_rays(KParams p, int sample, double* __restrict__ rays) {
  const size_t idx = (size_t)blockIdx.x * RM_BS + threadIdx.x;
  if (idx >= (size_t)p.nx * (size_t)p.nrows) return;
  const CameraDev& cam = *p.cam;
  const int row = (int)(idx / (size_t)p.nx), px_ = (int)(idx - (size_t)row * (size_t)p.nx);
  const int x = p.x0 + px_, y = p.y0 + row;
  const Ray r = lens_ray(cam, lens_target(cam, x, y), x, y, sample, p.seed);
  rm_store6(rays + 6 * idx, r.d, r.o);
}

// SPH: SPH_LIN_SCALAR, SPH_BVH_LDS (hierarchy nodes and leaf records staged in
// LDS) or SPH_BVH_GLOBAL.  att, paths, children, child_paths, leaves: may be null.
template <int SPH>
__global__ __launch_bounds__(RM_BS) void k_rt_map(KParams p, const double* __restrict__ rays,
                                                   const double* __restrict__ att, const int32_t* __restrict__ keys,
                                                   const uint64_t* __restrict__ paths, int32_t* __restrict__ info,
                                                   double* __restrict__ children, uint64_t* __restrict__ child_paths,
                                                   double* __restrict__ leaves) {
  const SceneDev& S = p.scene;                  // kernel argument: scalar loads
  extern __shared__ float4 lds_rm[];
  char* lds = reinterpret_cast<char*>(lds_rm);
  if (SPH == SPH_BVH_LDS) {
    const int nn = S.n_nodes * (int)(sizeof(Bvh4Node) / 16);
    for (int i = threadIdx.x; i < nn; i += RM_BS) lds_rm[i] = reinterpret_cast<const float4*>(S.bvh)[i];
    float4* leaf = reinterpret_cast<float4*>(lds + p.lds_leaf);
    for (int i = threadIdx.x; i < S.n_slots; i += RM_BS) leaf[i] = reinterpret_cast<const float4*>(S.bvh_sph32)[i];
    __syncthreads();                            // (the only barrier)
  }
  // A lane past the batch leaves before any walk: the hierarchy walk ballots over the lanes that entered it.
  const size_t i = (size_t)blockIdx.x * RM_BS + threadIdx.x;
  if (i >= (size_t)p.nrays) return;
  int* stk = reinterpret_cast<int*>(lds + p.lds_stack) + threadIdx.x;
  int* cov_i = reinterpret_cast<int*>(lds + p.lds_cov) + threadIdx.x;
  double* cov_v = reinterpret_cast<double*>(lds + p.lds_cov + COVER_K * RM_BS * 4) + threadIdx.x;

  const int pt = p.cam->pt;                     // monte_carlo_diffusion_times
  const int cmax = 2 + pt, lmax = S.n_light > 1 ? S.n_light : 1;
  const uint64_t R = (uint64_t)pt + 3;
  Item cur;
  cur.ray.d = v3p(rays + 6 * i);
  cur.ray.o = v3p(rays + 6 * i + 3);
  cur.att = att ? v3p(att + 3 * i) : v3(1.0, 1.0, 1.0);
  cur.path = paths ? paths[i] : 1;
  const int x = keys[4 * i], y = keys[4 * i + 1], sample = keys[4 * i + 2];
  cur.depth = keys[4 * i + 3];
  double* const ch = children ? children + i * (size_t)cmax * 9 : nullptr;
  uint64_t* const cp = child_paths ? child_paths + i * (size_t)cmax : nullptr;
  double* const lf = leaves ? leaves + i * (size_t)lmax * 3 : nullptr;

  // rt_map's raise sites, one word per group in the reference's order: high_lights, intersect,
  // intersect_parameters, local_lights' acos, path_tracing / local_lighting
  uint32_t errA = 0, errI = 0, errS = 0, errL = 0, errP = 0;
  int kind = 0, obj = -1, dir = -1, nch = 0, nleaf = 0;
  auto put = [&](const Ray& r, V3 a, uint64_t path) {
    if (ch) rm_store9(ch + 9 * nch, r.d, r.o, a);
    if (cp) cp[nch] = path;
    nch++;
  };

  const bool alive = !(cur.depth <= 0 || vr(cur.att) < 0.0001);   // rt_map's cutoff (ray_tracer.rb:52)
  bool fired = false;
  if (alive) {
    fired = highlight_leaves_att(
        S, cur.ray, [&] { return cur.att; },
        [&](V3 c) {
          if (lf) rm_store3(lf + 3 * nleaf, c);
          nleaf++;
        },
        errA, [&](V3 T, V3 L, double rad, int) { return raises_walk<SPH, RM_BS>(p, lds, T, L, rad); });
    kind = fired ? 1 : 2;
  }
  if (alive && !fired) {
    // ---- World#intersect (world.rb:37-59)
    double best = S.max_distance, total = 0.0;
    int besti = -1;
    bool hin = true;
    V3 hit = v3(0.0, 0.0, 0.0);
    if (SPH == SPH_LIN_SCALAR) {
      query<false>(S, cptr(S.sph32), true, cur.ray.o, cur.ray.d, hit, 0.0, best, besti, hit, hin, total, errI,
                   nullptr);
    } else {
      int q_ref = BVH_NONE, q_sp = 0, q_ncov = 0;
      bool q_ovf = false;
      if (SPH == SPH_BVH_LDS)
        query_bvh<RM_BS, false>(S, reinterpret_cast<const Bvh4Node*>(lds),
                                reinterpret_cast<const float4*>(lds + p.lds_leaf), S.bvh_sph64, S.bvh_obj, stk, cov_i,
                                cov_v, true, cur.ray.o, cur.ray.d, hit, 0.0, best, besti, hit, hin, total, errI, q_ref,
                                q_sp, q_ncov, q_ovf, false, 0);
      else
        query_bvh<RM_BS, false>(S, S.bvh, reinterpret_cast<const float4*>(S.bvh_sph32), S.bvh_sph64, S.bvh_obj, stk,
                                cov_i, cov_v, true, cur.ray.o, cur.ray.d, hit, 0.0, best, besti, hit, hin, total, errI,
                                q_ref, q_sp, q_ncov, q_ovf, false, 0);
    }
    if (besti >= 0) {
      const Material& m = S.mat[besti];
      V3 delta, n;
      hit_info(S, besti, cur.ray, hit, delta, n, hin);
      const V3 nn = vnorm(n, errS);             // n.normalize, shared by every use below
      const double c = vcos(cur.ray.d, n, errS);
      obj = besti;
      if (m.type == OBJ_SPHERE) {               // the direction World#intersect returns, as rtx_intersect
        dir = hin ? 0 : 1;
      } else {
        const double* plane = S.planes + (size_t)m.rec * PLANE_GEO;
        if (m.type == OBJ_BOX) {
          V3 h;
          int face = 0;
          box_hit(S.boxes + (size_t)m.rec * BOX_GEO, cur.ray.o, cur.ray.d, h, face);
          plane = S.boxes + (size_t)m.rec * BOX_GEO + face * PLANE_GEO;
        }
        dir = vdot(v3(plane[3], plane[4], plane[5]), cur.ray.d) < 0 ? 0 : 1;
      }
      // ---- World#local_lights (world.rb:72-80) fused with local_lighting's light loop
      // (world_object.rb:51-74): one SHADOW walk per light from hit + delta, then its term
      const V3 T = vadd(hit, delta);
      const bool xr = p.exact_raises != 0;      // the walk also checks its covers' acos raises (rtx_device.h xr_band)
      LightSum ls = {v3(0.0, 0.0, 0.0), 0};
      for (int li = 0; li < S.n_light; li++) {
        const LightDev& LD = S.light[li];
        const V3 L = v3p(LD.pos);
        const V3 d = vsub(L, T);                // Ray(light - target, target)
        double b2 = S.max_distance, tot = 1.0;
        int bi2 = -1;
        bool in2 = true;
        V3 h2 = v3(0.0, 0.0, 0.0);
        if (SPH == SPH_LIN_SCALAR) {
          query<false>(S, cptr(S.sph32), false, T, d, L, LD.radius, b2, bi2, h2, in2, tot, errL, nullptr, xr);
        } else {
          int q_ref = BVH_NONE, q_sp = 0, q_ncov = 0;
          bool q_ovf = false;
          if (SPH == SPH_BVH_LDS)
            query_bvh<RM_BS, false>(S, reinterpret_cast<const Bvh4Node*>(lds),
                                    reinterpret_cast<const float4*>(lds + p.lds_leaf), S.bvh_sph64, S.bvh_obj, stk,
                                    cov_i, cov_v, false, T, d, L, LD.radius, b2, bi2, h2, in2, tot, errL, q_ref, q_sp,
                                    q_ncov, q_ovf, false, 0, xr);
          else
            query_bvh<RM_BS, false>(S, S.bvh, reinterpret_cast<const float4*>(S.bvh_sph32), S.bvh_sph64, S.bvh_obj,
                                    stk, cov_i, cov_v, false, T, d, L, LD.radius, b2, bi2, h2, in2, tot, errL, q_ref,
                                    q_sp, q_ncov, q_ovf, false, 0, xr);
        }
        ls = light_term(S, LD, tot, hit, nn, ls.lc, ls.nl, errP);
      }
      // ---- the rest of rt_map (ray_tracer.rb:80-158), as shade_finish: every child is returned
      const Ray refl = reflection(cur.ray, nn, c, hit, delta, errS);
      put(refl, vmul(cur.att, v3p(m.refl_att)), cur.path * R + 1);
      Ray refr;
      bool has_refr = false;
      if (m.type == OBJ_SPHERE)                 // sphere.rb:92-94: rate inverted leaving
        has_refr = refraction(cur.ray, nn, c, hit, refl.d, hin ? m.rr : 1.0 / m.rr, refr, errS);
      else if (m.has_rr)                        // plane.rb:57-61: same rate both ways
        has_refr = refraction(cur.ray, nn, c, hit, refl.d, m.rr, refr, errS);
      if (has_refr) put(refr, vmul(cur.att, v3p(m.refr_att)), cur.path * R + 2);
      if (ls.nl == 0) {
        // WorldObject#path_tracing (world_object.rb:76-90) from hit + delta
        kind = 4;
        const V3 a = vmul(cur.att, vdiv_count(v3p(m.diffuse), pt));
        V3 left, up;
        pt_basis(n, nn, left, up, errP);
        Ray r;
        r.o = T;
        for (int k = 0; k < pt; k++) {
          r.d = pt_dir(p.seed, x, y, sample, cur.path, k, nn, left, up);
          put(r, a, cur.path * R + 3 + (uint64_t)k);
        }
      } else {
        kind = 3;
        const V3 leaf = vmul(cur.att, leaf_color(S, m, hit, ls.lc, ls.nl, errP));
        if (lf) rm_store3(lf, leaf);
        nleaf = 1;
      }
    }
  }

  // the first raise in the reference's order; a raising item returns nothing else
  uint32_t err = errA & 0xffu;
  if (!err) err = errI & 0xffu;
  if (!err) err = errS & 0xffu;
  if (!err) err = errL & 0xffu;
  if (!err) err = errP & 0xffu;
  double fill = 0.0;                            // unused slots: zeros
  if (err) {
    kind = -1;
    obj = dir = -1;
    nch = nleaf = 0;
    fill = __builtin_nan("");
  }
  const V3 f3 = v3(fill, fill, fill);
  for (int k = nch; k < cmax; k++) {
    if (ch) rm_store9(ch + 9 * k, f3, f3, f3);
    if (cp) cp[k] = 0;
  }
  if (lf)
    for (int k = nleaf; k < lmax; k++) rm_store3(lf + 3 * k, f3);
  int32_t* o = info + 6 * i;                    // 24-byte records
  if ((reinterpret_cast<uintptr_t>(info) & 7) == 0) {
    int2* o2 = reinterpret_cast<int2*>(o);
    o2[0] = make_int2(rm_status(err), kind);
    o2[1] = make_int2(obj, nch);
    o2[2] = make_int2(nleaf, dir);
  } else {
    o[0] = rm_status(err), o[1] = kind, o[2] = obj;
    o[3] = nch, o[4] = nleaf, o[5] = dir;
  }
}

hipError_t launch_lens_rays(const KParams& p, int32_t sample, double* d_rays, hipStream_t s) {
  if (p.nx <= 0 || p.nrows <= 0) return hipSuccess;
  const size_t n = (size_t)p.nx * (size_t)p.nrows;
  const dim3 grid((unsigned)((n + RM_BS - 1) / RM_BS));
  hipLaunchKernelGGL(k_lens_rays, grid, dim3(RM_BS), 0, s, p, (int)sample, d_rays);
  return hipGetLastError();
}

template <int SPH>
static hipError_t launch_rm(const KParams& p, size_t lds, const double* d_rays, const double* d_att,
                            const int32_t* d_keys, const uint64_t* d_paths, int32_t* d_info, double* d_children,
                            uint64_t* d_child_paths, double* d_leaves, hipStream_t s) {
  if (lds > 64 * 1024) {                        // deep traversal stacks: raise the kernel's dynamic-LDS limit once
    int cus, per_cu;
    const hipError_t e = launch_fit(reinterpret_cast<const void*>(k_rt_map<SPH>), RM_BS, lds, cus, per_cu);
    if (e != hipSuccess) return e;
  }
  const dim3 grid((unsigned)(((size_t)p.nrays + RM_BS - 1) / RM_BS));
  hipLaunchKernelGGL(k_rt_map<SPH>, grid, dim3(RM_BS), lds, s, p, d_rays, d_att, d_keys, d_paths, d_info, d_children,
                     d_child_paths, d_leaves);
  return hipGetLastError();
}

// Workgroups per CU the kernel's registers allow (216 / 217 VGPRs in the hierarchy
// variants: 2 waves per SIMD, 8 per CU): the hierarchy is staged only while its
// LDS image leaves that occupancy (the rule of LA_WGS_PER_CU, rtx_query.hip).
constexpr int RM_WGS_PER_CU = 2;

// mode: the context's SphMode.  The walks and the LDS image are launch_lit_area's
// (rtx_query.hip): a linear mode walks the ordered scan; every hierarchy mode
// walks the four-wide hierarchy, its nodes and leaf records staged in front of
// the traversal stacks and the cover lists when the hierarchy workgroup's layout
// holds them (resolve_mode) and this kernel's image fits RM_WGS_PER_CU times per
// CU; otherwise (C4) they are read from global memory.
hipError_t launch_rt_map(KParams p, int mode, const double* d_rays, const double* d_att, const int32_t* d_keys,
                         const uint64_t* d_paths, int32_t* d_info, double* d_children, uint64_t* d_child_paths,
                         double* d_leaves, hipStream_t s) {
  if (p.nrays <= 0) return hipSuccess;
  const SceneDev& S = p.scene;
  if (!sph_is_bvh(mode) || S.bvh_root == BVH_NONE)
    return launch_rm<SPH_LIN_SCALAR>(p, 0, d_rays, d_att, d_keys, d_paths, d_info, d_children, d_child_paths,
                                     d_leaves, s);
  const size_t stacks = (((size_t)S.bvh_stack * RM_BS * 4) + 15) & ~(size_t)15;
  const size_t covers = (size_t)COVER_K * RM_BS * 12;
  const size_t records = ((size_t)S.n_nodes * sizeof(Bvh4Node) + (size_t)S.n_slots * 16 + 15) & ~(size_t)15;
  const bool staged = mode != SPH_BVH_GLOBAL && resolve_mode(S, SPH_BVH_LDS) == SPH_BVH_LDS &&
                      records + stacks + covers <= LDS_TOTAL_BYTES / RM_WGS_PER_CU;
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
  return staged ? launch_rm<SPH_BVH_LDS>(p, off, d_rays, d_att, d_keys, d_paths, d_info, d_children, d_child_paths,
                                         d_leaves, s)
                : launch_rm<SPH_BVH_GLOBAL>(p, off, d_rays, d_att, d_keys, d_paths, d_info, d_children,
                                            d_child_paths, d_leaves, s);
}

}  // namespace rtx
