// rtx_plan.h — the launch plan of the bounce-level engine:
// the sphere mode, the hit ring, where the light buffer and the raise gates
// sit, the raise-check variant, the workgroup's claim counter and the dynamic
// LDS bytes a fused level launch ends up with.  Host-only arithmetic over
// SceneDev's scalars and a few option values, plain C++ (g++ -std=c++17, as
// rtx_scene_build.h and rtx_sched.h): the launchers (rtx_kernels.hip,
// rtx_levels.hip), rtx_capi.cpp and tools/scene_dump.cpp all call this one copy.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "rtx_scene.h"

namespace rtx {

// Where the sphere walk reads its records:
enum SphMode : int {
  SPH_LIN_LDS = 0,       // ordered linear walk, float32 pre-test records staged in LDS
  SPH_LIN_SCALAR = 1,    // ordered linear walk, records by scalar loads
  SPH_BVH_LDS = 2,       // four-wide ball hierarchy, nodes + leaf records staged in LDS
  SPH_BVH_GLOBAL = 3,    // four-wide ball hierarchy, nodes + leaf records by scalar loads
  SPH_BVH_MIX = 4,       // four-wide ball hierarchy, nodes staged in LDS, leaf records from global memory
                         // (bounce-level engine only: room for the hit rings of k_level_c; the lanes
                         // engine walks it as SPH_BVH_LDS)
  SPH_BVH_LDSX = 5,      // as SPH_BVH_LDS, and the binary64 sphere records of the exact test with their
                         // object indices staged too (bounce-level engine only, small hierarchies: no
                         // global load inside the walk; the lanes engine walks it as SPH_BVH_LDS)
  SPH_BVH_QLDS = 6,      // four-wide ball hierarchy, nodes + 16-bit quantized leaf records (SceneDev::bvh_q)
                         // in LDS, 16-bit traversal stacks (bounce-level engine only, hierarchies too big for
                         // SPH_BVH_LDS next to a hit ring, e.g. C4; the lanes engine walks it as SPH_BVH_LDS)
};

// Sphere modes that walk the ball hierarchy.
constexpr bool sph_is_bvh(int m) {
  return m == SPH_BVH_LDS || m == SPH_BVH_GLOBAL || m == SPH_BVH_MIX || m == SPH_BVH_LDSX || m == SPH_BVH_QLDS;
}

// LDS budgets.  Linear walk: 16 B per sphere in 256-thread workgroups, small
// enough for several workgroups per CU.  Hierarchy: nodes + leaf records in
// one 512-thread workgroup per CU (2 waves per SIMD, the register-limited
// occupancy), next to its stacks and cover lists.
constexpr size_t LDS_SPHERE_BYTES = 32 * 1024;
constexpr size_t LDS_LIN_BLOCK_BYTES = 76 * 1024;   // two 256-thread workgroups per CU
constexpr int BS_LIN = 256;                         // (LDS_TOTAL_BYTES, BS_BVH: rtx_scene.h)
constexpr int ITEM_WORDS = 11;                      // doubles per ray-stack entry (rtx_device.h RayStack)

// The hit rings of k_level_c (rtx_levels.hip): LV_RING slots per wave, LV_RING_FIELDS
// doubles per parked hit, or LV_RING_FIELDS_SMALL in the compact ring.
constexpr int LV_RING = 128;
constexpr int LV_RING_FIELDS = 11;
constexpr int LV_RING_FIELDS_SMALL = 5;
constexpr size_t LV_RING_WAVE_BYTES = (size_t)LV_RING * LV_RING_FIELDS * 8;
constexpr size_t LV_RING_WAVE_BYTES_SMALL = (size_t)LV_RING * LV_RING_FIELDS_SMALL * 8;

constexpr int LV_SPLIT_MAX_LIGHTS = 16;         // split phases only up to this many lights (shadow results per hit)

// The raise check of a launch's shadow walks (option exact_raises, rtx_levels.hip lv_walk).
enum { XR_NONE = 0, XR_BUF = 1, XR_WALK = 2 };

// The options a plan reads, with the context's defaults (rtx_capi.cpp takes its own from here).
struct PlanOpts {
  int bvh = 1;             // 0: ordered linear walk; 1: hierarchy from bvh_min spheres; 2: always
  int bvh_min = 32;        // C2 (64 spheres): hierarchy 16.0 ms vs ordered walk 17.8 ms
  int sphere_src = -1;     // 0 LDS staging, 1 scalar loads, 2 nodes LDS + leaves global, 3 + exact records in LDS,
                           // 4 quantized leaves in LDS, -1 auto
  int lv_compact = -1;     // 1 = park hits in an LDS ring and shade full waves, -1 auto (when it fits), 2 compact ring
  int lv_split = 0;        // 1 = three phase launches per level
  int lbuf = 1;            // 1 = shadow walks through the light buffer where it is staged (§3.18)
  int exact_raises = 1;    // 1 = shadow walks also check the acos raises of the covers they skip
};

// Sphere walk the options ask for (SphMode); resolve_mode falls back to scalar
// loads when the records exceed the LDS budget.
inline int sph_mode_of(const SceneDev& S, int bvh, int bvh_min, int sphere_src) {
  const bool hier = bvh == 2 || (bvh == 1 && S.n_sphere >= bvh_min);
  if (hier && S.bvh_root != BVH_NONE)
    return sphere_src == 4   ? SPH_BVH_QLDS
           : sphere_src == 3 ? SPH_BVH_LDSX
           : sphere_src == 2 ? SPH_BVH_MIX
           : sphere_src == 1 ? SPH_BVH_GLOBAL
                             : SPH_BVH_LDS;
  return sphere_src == 1 ? SPH_LIN_SCALAR : SPH_LIN_LDS;
}

// The bounce-level engine's sphere mode for sphere_src auto: SPH_BVH_LDSX
// when the hierarchy, its exact records and the full hit ring fit LDS (C2);
// SPH_BVH_MIX when the staged hierarchy leaves no LDS for a hit ring while
// the hierarchy's nodes alone with the compact ring fit (C4); else SPH_BVH_LDS.
inline int levels_auto_mode(const SceneDev& S, int mode, int compact, int split) {
  if (mode != SPH_BVH_LDS || compact == 0 || split) return mode;
  const size_t waves = BS_BVH / 64;
  const size_t walk = (size_t)S.bvh_stack * BS_BVH * 4 + (size_t)COVER_K * BS_BVH * 12 + 64;
  const size_t nodes = (size_t)S.n_nodes * sizeof(Bvh4Node), leaves = (size_t)S.n_slots * 16;
  const size_t exact = (size_t)S.n_slots * (sizeof(Sphere64) + 4) + 16 + (size_t)S.n_obj * sizeof(Material) +
                       (size_t)S.n_sphere * sizeof(Sphere64);   // + shading's materials and sphere records
  // C2: the exact test's records staged too (r05d: 4.91-4.94 -> 4.85 ms, same bits)
  if (nodes + leaves + exact + walk + waves * LV_RING_WAVE_BYTES <= LDS_TOTAL_BYTES) return SPH_BVH_LDSX;
  if (nodes + leaves + walk + waves * LV_RING_WAVE_BYTES <= LDS_TOTAL_BYTES) return mode;   // LDS + full ring
  if (nodes + leaves + walk + waves * LV_RING_WAVE_BYTES_SMALL <= LDS_TOTAL_BYTES) return mode;   // + compact ring
  // C4: the leaves as 16-bit records, 16-bit stacks (+ alignment)
  const size_t walk16 = (size_t)S.bvh_stack * BS_BVH * 2 + (size_t)COVER_K * BS_BVH * 12 + 64;
  if (S.q_ok && nodes + (size_t)S.n_slots * 8 + walk16 + 32 + waves * LV_RING_WAVE_BYTES_SMALL <= LDS_TOTAL_BYTES)
    return SPH_BVH_QLDS;
  if (nodes + walk + waves * LV_RING_WAVE_BYTES_SMALL <= LDS_TOTAL_BYTES) return SPH_BVH_MIX;
  return mode;
}

// mode: SphMode; a linear mode whose records exceed the LDS budget falls back to
// SPH_LIN_SCALAR, a hierarchy mode to a smaller staging or SPH_BVH_GLOBAL
// (its budget: rtx_scene.h bvh_lds_bytes / bvh_lds_budget).
inline int resolve_mode(const SceneDev& S, int mode) {
  if (mode == SPH_BVH_QLDS) {                  // nodes + 16-bit leaf records + 16-bit stacks, when conservative
    const size_t need = (size_t)S.n_nodes * sizeof(Bvh4Node) + (size_t)S.n_slots * 8 +
                        (size_t)S.bvh_stack * BS_BVH * 2 + (size_t)COVER_K * BS_BVH * 12 + 64;
    if (S.q_ok && need <= LDS_TOTAL_BYTES) return mode;
    mode = SPH_BVH_MIX;
  }
  if (mode == SPH_BVH_LDSX) {                  // the staged hierarchy plus its exact records
    const size_t need = bvh_lds_bytes(S.n_nodes, S.n_slots, S.bvh_stack) + (size_t)S.n_slots * (sizeof(Sphere64) + 4) +
                        16 + (size_t)S.n_obj * sizeof(Material) + (size_t)S.n_sphere * sizeof(Sphere64);
    if (need <= LDS_TOTAL_BYTES) return mode;
    mode = SPH_BVH_LDS;
  }
  if (mode == SPH_BVH_MIX) {                   // nodes in LDS, leaves global: needs room for the nodes
    const size_t need = (size_t)S.n_nodes * sizeof(Bvh4Node) + (size_t)S.bvh_stack * BS_BVH * 4 +
                        (size_t)COVER_K * BS_BVH * 12 + 64;
    return need > LDS_TOTAL_BYTES ? SPH_BVH_GLOBAL : SPH_BVH_MIX;
  }
  if (mode == SPH_LIN_LDS && (size_t)(S.n_sphere + 4) * 16 > LDS_SPHERE_BYTES) return SPH_LIN_SCALAR;
  if (mode == SPH_BVH_LDS && bvh_lds_bytes(S.n_nodes, S.n_slots, S.bvh_stack) > LDS_TOTAL_BYTES)
    return SPH_BVH_GLOBAL;
  return mode;
}

// The walk's part of a workgroup's dynamic LDS for `mode` (byte offsets, -1: not
// staged) and its size; rtx_device.h lds_layout copies it into KParams.
struct WalkLds {
  int32_t stack = 0, cov = 0, items = 0;
  int32_t leaf = -1, x64 = -1, xobj = -1, mat = -1, sphr = -1;
  int32_t stk_slots = 0;
  size_t bytes = 0;
};
inline WalkLds walk_lds(const SceneDev& S, int mode, int bs, int stk_slots_max) {
  WalkLds w;
  size_t off = 0;
  if (mode == SPH_LIN_LDS) off = (size_t)(S.n_sphere + 4) * 16;
  if (mode == SPH_BVH_LDS || mode == SPH_BVH_MIX || mode == SPH_BVH_LDSX || mode == SPH_BVH_QLDS) {
    off = (size_t)S.n_nodes * sizeof(Bvh4Node);
    w.leaf = (int32_t)off;
    if (mode == SPH_BVH_QLDS) off += (size_t)S.n_slots * 8;   // 16-bit records
    else if (mode != SPH_BVH_MIX) off += (size_t)S.n_slots * 16;
    if (mode == SPH_BVH_LDSX) {
      w.x64 = (int32_t)off;
      off += (size_t)S.n_slots * sizeof(Sphere64);
      w.xobj = (int32_t)off;
      off += (size_t)S.n_slots * 4;
      off = (off + 15) & ~(size_t)15;
      w.mat = (int32_t)off;                     // shading's material and sphere record of the hit object
      off += (size_t)S.n_obj * sizeof(Material);
      w.sphr = (int32_t)off;
      off += (size_t)S.n_sphere * sizeof(Sphere64);
    }
  }
  off = (off + 15) & ~(size_t)15;
  w.stack = (int32_t)off;
  w.cov = (int32_t)off;
  if (sph_is_bvh(mode)) {
    off += (size_t)S.bvh_stack * bs * (mode == SPH_BVH_QLDS ? 2 : 4);   // QLDS: int16 entries
    off = (off + 15) & ~(size_t)15;
    w.cov = (int32_t)off;
    off += (size_t)COVER_K * bs * 12;
  }
  // the bottom of every lane's ray stack, as many entries as fit the budget
  off = (off + 15) & ~(size_t)15;
  w.items = (int32_t)off;
  const size_t budget = sph_is_bvh(mode) ? LDS_TOTAL_BYTES : LDS_LIN_BLOCK_BYTES;
  const size_t per = (size_t)ITEM_WORDS * 8 * bs;
  int slots = budget > off ? (int)((budget - off) / per) : 0;
  if (slots > stk_slots_max) slots = stk_slots_max;
  w.stk_slots = slots;
  off += (size_t)slots * per;
  w.bytes = off;
  return w;
}

// What a level launch of the bounce-level engine settles before it picks its kernel.
struct LevelPlan {
  int mode = 0;            // the launch's sphere mode (resolved)
  WalkLds walk;            // (no ray stack in this engine: stk_slots 0)
  int ring_fields = 0;     // hit ring: 0 none (k_level), LV_RING_FIELDS full, LV_RING_FIELDS_SMALL compact (k_level_c)
  int xrm = XR_NONE;       // XR_NONE / XR_BUF / XR_WALK
  int32_t lds_ring = -1, lds_lbuf = -1, lds_rgate = -1;   // byte offsets, -1: absent
  int32_t lds_sched = -1;  // the workgroup's claim counter, -1: no room (the launch runs lv_round 0)
  size_t lds = 0;          // dynamic LDS bytes of the launch
};

// The values of `o` a level launch reads, and whether the scene's light and raise buffers were uploaded.
struct PlanIn {
  int lv_compact, lbuf, exact_raises;
  bool have_lbuf, have_rbuf;
};
// rtx_scene_upload ships the light buffer when it was built, the raise buffer and its gates likewise.
inline PlanIn plan_in(const SceneDev& host, const PlanOpts& o) {
  return PlanIn{o.lv_compact, o.lbuf, o.exact_raises, host.lbuf_n != 0, host.rbuf_n != 0};
}

// kind: 0 k_level / k_level_c (fused), 1 k_lv_trace, 2 k_lv_shadow; fused_bs: `bs` is the fused
// kernel's block size (k_level_c is instantiated for that one only).  The kernel variants of a level
// that is the batch's last, or binned (lv_sort), share this plan: neither changes a value here.
inline LevelPlan level_plan(const SceneDev& S, const PlanIn& in, int mode, int bs, bool fused_bs, int kind) {
  LevelPlan pl;
  pl.mode = mode;
  pl.walk = walk_lds(S, mode, bs, 0);
  size_t lds = pl.walk.bytes;
  const bool bvh = sph_is_bvh(mode);
  const size_t budget = bvh ? LDS_TOTAL_BYTES : LDS_LIN_BLOCK_BYTES;
  // exact_raises (the default) compiles the shadow walks' raise check in (k_level / k_level_c <..., XR>):
  // XR_BUF through the light and raise buffers where both serve this launch (the LDS-staged light
  // buffer of SPH_BVH_LDSX, the global one of SPH_BVH_QLDS), else XR_WALK; exact_raises = 0: XR_NONE
  const bool xr = in.exact_raises != 0;
  const bool bufs = mode == SPH_BVH_QLDS && in.lbuf && in.have_lbuf && in.have_rbuf;   // (SPH_BVH_LDSX: settled below)
  pl.xrm = !xr ? XR_NONE : bufs ? XR_BUF : XR_WALK;
  // hit compaction when the rings fit next to the walk's LDS
  if (fused_bs && kind == 0 && in.lv_compact != 0) {
    const size_t ring = (lds + 15) & ~(size_t)15;
    const size_t need = ring + (size_t)(bs / 64) * LV_RING_WAVE_BYTES;
    const size_t need_small = ring + (size_t)(bs / 64) * LV_RING_WAVE_BYTES_SMALL;
    if (need <= budget && in.lv_compact != 2) {   // the full ring
      pl.lds_ring = (int32_t)ring;
      lds = need;
      pl.ring_fields = LV_RING_FIELDS;
    } else if (bvh && need_small <= budget) {  // the compact ring (C4-sized hierarchies)
      pl.lds_ring = (int32_t)ring;
      lds = need_small;
      pl.ring_fields = LV_RING_FIELDS_SMALL;
    }
  }
  // the light buffer (§3.18) after the rings, when it fits: the shadow walks read their cell's leaves;
  // with exact_raises the raise buffer's gates after it (§2.4), in LDS when they fit too
  if (mode == SPH_BVH_LDSX && kind == 0 && in.lbuf && in.have_lbuf) {
    const size_t at = (lds + 15) & ~(size_t)15, bytes = (size_t)S.lbuf_stride * S.n_light * 2;
    if (at + bytes <= LDS_TOTAL_BYTES) {
      pl.lds_lbuf = (int32_t)at;
      lds = at + bytes;
      if (xr && in.have_rbuf) {
        pl.xrm = XR_BUF;
        const size_t ga = (lds + 15) & ~(size_t)15, gb = (size_t)S.rgate_stride * S.n_light * 2;
        if (ga + gb <= LDS_TOTAL_BYTES) {
          pl.lds_rgate = (int32_t)ga;
          lds = ga + gb;
        }
      }
    }
  }
  if (fused_bs && pl.ring_fields == 0 && kind == 0 && pl.xrm == XR_BUF) {   // (no ring: k_level, which walks the
    pl.xrm = XR_WALK;                                                       //  widened hierarchy)
    pl.lds_lbuf = pl.lds_rgate = -1;
  }
  // rounds (lv_round): the workgroup's claim counter after everything else; where the layout leaves no
  // room for it, this launch keeps the per-wave static schedule (placed whatever lv_round is: a kernel's
  // dynamic LDS size, which launch_fit caches and raises the kernel's limit to, does not depend on the option)
  const size_t at = (lds + 3) & ~(size_t)3;
  if (at + 4 <= budget) {
    pl.lds_sched = (int32_t)at;
    lds = at + 4;
  }
  pl.lds = lds;
  return pl;
}

// A plan in one integer (read-only option lv_plan_last, scene_dump --plan): bits 0-3 the sphere mode,
// 4-7 the ring fields, 8 light buffer in LDS, 9 raise gates in LDS, 10-11 the xr mode, 12 claim counter
// placed, 16 and up the dynamic LDS bytes.
inline int64_t pack_plan(const LevelPlan& pl) {
  return (int64_t)pl.mode | (int64_t)pl.ring_fields << 4 | (int64_t)(pl.lds_lbuf >= 0) << 8 |
         (int64_t)(pl.lds_rgate >= 0) << 9 | (int64_t)pl.xrm << 10 | (int64_t)(pl.lds_sched >= 0) << 12 |
         (int64_t)pl.lds << 16;
}

// The plan of the fused level launches of a render with the options `o` (the sphere mode as
// render_levels settles it, then launch_levels' resolve_mode); -1 when the split phases run instead.
inline int64_t fused_plan(const SceneDev& host, const PlanOpts& o) {
  if (o.lv_split != 0 && host.n_light <= LV_SPLIT_MAX_LIGHTS) return -1;
  int mode = sph_mode_of(host, o.bvh, o.bvh_min, o.sphere_src);
  if (o.sphere_src == -1) mode = levels_auto_mode(host, mode, o.lv_compact, o.lv_split);
  mode = resolve_mode(host, mode);
  return pack_plan(level_plan(host, plan_in(host, o), mode, sph_is_bvh(mode) ? BS_BVH : BS_LIN, true, 0));
}

}  // namespace rtx
