// rtx_launch.h — kernel parameter block and launchers shared by the C-ABI
// (rtx_capi.cpp) and the kernels (rtx_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rtx_batch.h"
#include "rtx_plan.h"
#include "rtx_scene.h"

namespace rtx {

// Reference raise sites recorded by the device (codes: ERR_* in rtx_vec3.h).
struct ErrState {
  unsigned int flags;              // bit (1 << code) for every code raised
  unsigned int pad;
  unsigned long long first[5];     // per ERR_ code (rtx_vec3.h): min key (pixels: (x*H + y)*2 + phase, render_sync order; rays: index)
};

// (LV_MAXL, LV_SLICES, ..., LevelCtl, RAY_BYTES, levels_rec_bytes and the batch layout: rtx_batch.h, host-only)

struct KParams {
  SceneDev scene;                  // by value: read by scalar loads from the kernarg segment
  const CameraDev* cam;            // device copy (uploaded by rtx_camera_set)
  uint64_t seed;
  int32_t x0, nx, nrows;           // columns [x0, x0+nx); packed output rows
  int32_t y0, tile_rows, rank, nranks;   // tile_rows == 0: rows y0 .. y0+nrows-1
  const int32_t* row_tiles;        // non-null: packed tile k is image tile row_tiles[k] (rtx_render_tile_list_device)
  uint32_t* tile_rays;             // non-null (whole-frame level renders): rays per 8x8 tile, written by the reduction
  double* out;
  size_t stride;                   // doubles per output row
  ErrState* err;
  unsigned long long* counts;      // RTX_NCOUNT counters (counting launches only)
  int* work;                       // work-item counter of this launch (zeroed by the launcher)
  const double* rays;              // SRC_RAYS (rtx_trace): 6 doubles per ray, keys (x, y, sample)
  const int32_t* keys;
  int32_t nrays;
  // dynamic LDS layout (bytes), filled by launch_render/launch_trace
  int32_t lds_leaf, lds_stack, lds_cov, lds_items;
  int32_t lds_x64, lds_xobj;       // SPH_BVH_LDSX: staged Sphere64 records / object indices per leaf slot
  int32_t lds_lbuf;                // the light buffer staged in LDS (byte offset), or -1: shadow walks use the hierarchy
  int32_t lds_rgate;               // the raise buffer's gates staged in LDS (byte offset), or -1: read from global memory
  int32_t lds_mat, lds_sphr;       // SPH_BVH_LDSX: staged materials (per object) / Sphere64 records (per sphere)
  int32_t stk_slots;               // ray-stack entries per lane kept in LDS (set by the launcher)
  int32_t stk_slots_max;           // cap (option "lds_stack"; the stack bucket by default)
  double* stk_glb;                 // per-lane regions: lanes_maxs * 12 doubles of ray stack
  int32_t lanes_maxs;              // lanes engine: ray-stack entries per lane (8, 16, 32 or 64; set by the launcher)
  int32_t stk_glb_lanes;           // lanes the buffer holds (the launcher caps the grid to it)
  // Camera#render_at in two steps (launch_render): per (pixel, sample) records
  // of 4 doubles {r, g, b, first raise} at samples[(pixel * max(pre, max) + j) * 4]
  // (pixel = row * nx + column of the region), and the list of pixels whose
  // variance asks for the extra samples.
  int32_t pre, max_samples;        // camera pre_sample_times / max_sample_times
  int32_t postpone;                // query_bvh: postpone walks when fewer lanes than this still walk (0: never)
  double* samples;
  int32_t* extra_list;             // nx * nrows entries
  int32_t* extra_count;
  // SRC_PIXELS: tile visiting order (k_tile_cost + k_tile_sort), null = natural
  int32_t* tile_order;
  int32_t* tile_cls;
  // bounce-level engine: one batch = pass 0 (the pre samples of the pixels of
  // tiles lv_t0 + k * lv_tstride, k < lv_tiles) or pass 1 (the extra samples of extra-list
  // entries [lv_e0, lv_e0 + lv_entries)); level-0 item k of the batch is
  // decode_item(k); trees are stored per level in lv_rec (lv_rec_bytes each).
  int32_t lv_pass, lv_t0, lv_tiles, lv_e0, lv_entries;
  int32_t lv_tstride;              // 1, or 2 for the interleaved halves of a two-stream render
  uint32_t lv_scap;                // ray records per staging buffer (levels >= 1): LV_SLICES << lv_slice_log2
  int32_t lv_slice_log2;           // slots per slice of a level's ray queue (log2)
  int32_t lv_hslice_log2;          // split phases: slots per slice of a level's hit queue (log2)
  uint32_t lv_lcap;                // tree records in lv_rec
  int32_t lv_rec_bytes;
  LevelCtl* lv_ctl;
  double* lv_stage[2];             // level d reads lv_stage[d & 1], writes lv_stage[(d + 1) & 1]
  char* lv_rec;
  int32_t* lv_redo_of;             // per level-0 item: -1, or its entry in lv_redo_list
  int32_t* lv_redo_list;           // level-0 items re-rendered by the lanes engine (SRC_LIST)
  double* lv_redo_smp;             // their sample records {r, g, b, first raise}
  unsigned long long* lv_acc;      // per call: {redo_n, dropped, count[0..LV_MAXL]} summed over batches (or null)
  int32_t lv_split;                // 1: three phase launches per level (k_lv_trace / k_lv_shadow / k_lv_shade)
  int32_t lv_static_pct;           // % of a level launch's chunks scheduled statically (the rest: sharded claims)
  int32_t lv_round;                // static chunks: 0 wave w takes w, w + W, ...; R > 0 rounds of R chunks per workgroup,
                                   // claimed from the LDS word at lds_sched (option lv_round; the launcher clears it
                                   // where that word finds no room)
  int32_t lds_sched;               // LDS byte offset of the workgroup's claim counter (lv_round > 0)
  double* lv_hit;                  // split: hit queue, LV_HIT_BYTES per hit, LV_SLICES << lv_hslice_log2 slots
  double* lv_area;                 // split: {1 - covers, raise} per (hit, light)
  int32_t lv_compact;              // k_level: park hits in an LDS ring, shade full waves (-1 auto, 0 off, 1 on, 2 compact ring)
  int32_t lds_ring;                // k_level (compacting): LDS byte offset of the per-wave hit rings
  int32_t lv_last_level;           // trace_depth - 1 (-1 if trace_depth < 1): the level whose children are all
                                   // cut off, run by a k_level_c compiled for it
  int32_t lv_grid_div;             // level launches: persistent grid = resident workgroups / this (option lv_grid_div)
  int32_t lv_fin_tiles;            // tree reduction pass 0: tiles of the batch (grid-stride loop when the grid is smaller)
  int32_t lv_redo_blocks;          // the lanes-engine re-render of overflowed samples: at most this many workgroups (0: all resident)
  int32_t lv_ray_dbl;              // staged ray record, doubles: 10 (80 B: path < 2^32, RNG key decoded from the root) or 12
  int32_t exact_raises;            // 1: every shadow walk (local_lights) also checks its covers' acos raises (option exact_raises)
  uint32_t lv_hlq_cap;             // entries of lv_hlq
  double* lv_hlq;                  // highlight rays of the batch whose lit_area raise k_hl_raise checks (8 doubles each)
  // ray binning (option lv_sort): a level >= 1 is processed in the order of its
  // rays' bins (lv_ray_bin: direction octant, origin cell), records still at
  // their dense index
  int32_t lv_sort;                 // 0, or the first level binned before its launch (option lv_sort_from)
  int32_t lv_cell_bits;            // origin cells per axis of a bin = 2^lv_cell_bits (3 or 4: 4,096 or 32,768 bins)
  int32_t lv_lbuf;                 // 1: the fused level kernels' shadow walks use the light buffer when staged (option lbuf)
  uint16_t* lv_key;                // bin of each staged ray of the level being binned, by queue slot (k_lv_bin)
  uint2* lv_perm;                  // the level's rays in bin order: {queue slot, dense index}
  double* lv_sorted;               // lv_sort_copy: the binned level's ray records in bin order (k_lv_bin), or null
  uint32_t* lv_bins;               // LV_BINS counts, LV_BINS cursors (the first 8 << 3 lv_cell_bits used)
};

// (SphMode, sph_is_bvh, levels_auto_mode, resolve_mode and the level launch plan: rtx_plan.h, host-only)

// HIP event pairs recorded on the launch stream around every ray-tree kernel
// launch of one render call (option "kernel_events", rtx_kernel_time).
struct KernelEvents {
  hipEvent_t* ev;                  // 2 * max events: start, end of launch k at ev[2k], ev[2k+1]
  int n, max;
};

int stack_bucket(int need);
// Persistent-launch occupancy (CUs, resident blocks per CU) of `kern`, cached
// per (kernel, block size, dynamic LDS bytes, device); raises the kernel's
// dynamic-LDS limit on first use.
hipError_t launch_fit(const void* kern, int bs, size_t lds, int& cus, int& per_cu);
// mode: SphMode, resolved by rtx_plan.h resolve_mode.  Counting launches always walk
// linearly (the counters are the reference's brute-force events).
hipError_t launch_render(KParams p, int mode, bool count, int maxs, hipStream_t s, KernelEvents* kev = nullptr);
hipError_t launch_trace(KParams p, int mode, int maxs, hipStream_t s);
// Camera#render_at over the region of `p` with the bounce-level engine: nlev =
// trace_depth level launches per batch of `batch_tiles` 8x8 tiles (pass 0) or
// of batch_tiles * 64 * pre / (max - pre) extra-list entries (pass 1).  The
// lv_* buffers of `p` are the caller's: lv_redo_of / lv_rec / staging sized for
// batch_tiles * 64 * pre level-0 items; lanes-engine buffers (stk_glb) too, for
// the overflow re-render.
// Parts at once (option lv_streams = P > 1): pass 0's tiles interleaved over
// P parts, tile t in part t mod P; part 0 on `s` with the buffers of `p`,
// part j > 0 on s2[j - 1] with the buffers of pb[j - 1] (own level buffers,
// work counter and lanes-engine stacks; the extra-sample list and the
// statistics shared with `p`).  The parts j > 0 start after the first reset
// on `s` (ev_first); `s` waits for all of them (ev_done) before the extra
// samples (pass 1), which run on `s` alone.
struct LvAux {
  int parts;                       // P (2 .. LV_MAX_PARTS)
  KParams pb[LV_MAX_PARTS - 1];
  hipStream_t s2[LV_MAX_PARTS - 1];
  hipEvent_t ev_first, ev_done[LV_MAX_PARTS - 1];
};
hipError_t launch_levels(KParams p, int mode, int maxs, int nlev, int batch_tiles, hipStream_t s,
                         KernelEvents* kev = nullptr, const LvAux* aux = nullptr, int64_t* plan_out = nullptr);
// (plan_out: receives rtx_plan.h pack_plan of the call's first fused level launch, as launched)
hipError_t launch_path_trace(KParams p, hipStream_t s);
// The lanes engine's re-render of the level-0 items listed in lv_redo_list
// (SRC_LIST; exits at once when the list is empty).
hipError_t launch_redo(const KParams& q, int mode, int maxs, int n, hipStream_t s);
// The same for a trace call's batch: the explicit rays listed in lv_redo_list (SRC_RAYLIST).
hipError_t launch_redo_rays(const KParams& q, int mode, int maxs, int n, hipStream_t s);
// RayTracer#trace_sync for the p.nrays explicit rays p.rays / p.keys (device buffers) -> p.out [n][3] and
// status int32[n] (or null), in batches of `batch` rays.  levels: through the bounce
// levels (the lv_* buffers of `p` sized for `batch` level-0 items, 96-B staged records, no split phases);
// else every ray through the lanes engine (lv_ctl and the lv_redo_* buffers only).  Nothing goes to p.err.
// live: null, or the number of rays that exist, in device memory (<= p.nrays, the capacity the launches are
// sized for): slots at or past it are padding, with no tree, no status and no colour written.  first false:
// the call adds to the level statistics of the calls before it instead of resetting them.
hipError_t launch_trace_levels(KParams p, int mode, int maxs, int nlev, int batch, bool levels, int32_t* status,
                               hipStream_t s, KernelEvents* kev = nullptr, int64_t* plan_out = nullptr,
                               const int32_t* live = nullptr, bool first = true);
// Camera#render_at for a list of pixels (rtx_render_pixels, DESIGN.md §3.23, rtx_pixels.hip).  One chunk's
// buffers: rays [cap][6], keys int32[cap][3], the traced samples' colours col [cap][3] and statuses st
// int32[cap] (cap = pixels x max(pre, max - pre)), the pixels taking extra samples list int32[pixels] and
// count int32[2] = {listed pixels, their extra samples}.
struct PixelBufs {
  double* rays;
  int32_t* keys;
  double* col;
  int32_t* st;
  int32_t* list;
  int32_t* count;
};
// The lens rays and keys (x, y, j), j < pre, of the npx pixels d_xy, item (pixel, sample); zeroes the count.
hipError_t launch_pixel_rays(const CameraDev* cam, uint64_t seed, const int32_t* d_xy, int npx, int pre,
                             const PixelBufs& b, hipStream_t s);
// render_at's pixel stage over the traced pre samples (col, st): rgb [npx][3], variance [npx] or null, info
// int32[npx][2] = {status, samples} or null; the pixels whose variance asks for extra samples are listed.
hipError_t launch_pixel_reduce(const CameraDev* cam, int npx, int pre, int max_samples, const PixelBufs& b,
                               double* d_rgb, double* d_variance, int32_t* d_info, hipStream_t s);
// The rays and keys (x, y, j), j = pre .. max - 1, of the listed pixels, item (list entry, sample); count[1].
hipError_t launch_pixel_extra_rays(const CameraDev* cam, uint64_t seed, const int32_t* d_xy, int npx, int pre,
                                   int max_samples, const PixelBufs& b, hipStream_t s);
// The listed pixels' colours from the pre mean parked in d_rgb and the traced extra samples (col, st).
hipError_t launch_pixel_finish(int npx, int pre, int max_samples, const PixelBufs& b, double* d_rgb, int32_t* d_info,
                               hipStream_t s);
int read_level_stamps(unsigned long long* out, int reset);   // diagnostic builds
hipError_t launch_quantize(const double* rgb, int w, int h, size_t stride, int blend, uint8_t* out,
                           hipStream_t s);
// Rank-major packed tiles (n ranks x rows_per_rank rows x w x 3) -> frame rows.
hipError_t launch_unpack(const double* gathered, int w, int h, int tile_rows, int n, int rows_per_rank,
                         double* out, size_t stride, hipStream_t s);
hipError_t launch_unpack_plan(const double* gathered, int w, int h, int tile_rows, int n, int per_rank,
                              const int32_t* d_plan, double* out, size_t stride, hipStream_t s);
hipError_t launch_tile_probe(KParams p, int32_t* cls, hipStream_t s);
// First-hit feature buffers of the region of `p` for camera sample `sample`
// (rtx_aov.hip): d_ids int32[nrows][nx][3], d_geom double[nrows][nx][10];
// either may be null.  mode: SphMode (a hierarchy mode walks the hierarchy,
// staged in LDS when it fits, else from global memory).
hipError_t launch_first_hit(KParams p, int mode, int32_t sample, int32_t* d_ids, double* d_geom, hipStream_t s);
// Batched World queries over p.nrays items; p.cam is unused.
// World#intersect of the rays p.rays (rtx_aov.hip): d_ids int32[n][3], d_geom
// double[n][13] (launch_first_hit's ten values, then delta); either may be null.
hipError_t launch_intersect(KParams p, int mode, int32_t* d_ids, double* d_geom, hipStream_t s);
// World#lit_area / #local_lights of the targets d_targets [n][3] (rtx_query.hip)
// against the scene's lights (d_lights null: L = n_light entries per target) or
// one explicit light {position, radius} each (d_lights [n][4], L = 1): d_area
// [n][L], d_color [n][L][3] or null, d_status int32[n] or null (the rtx_status
// of the target's first raise; nothing goes to p.err).
hipError_t launch_lit_area(KParams p, int mode, const double* d_targets, const double* d_lights, double* d_area,
                           double* d_color, int32_t* d_status, hipStream_t s);
// Batched Camera#lens_func and RayTracer#rt_map (rtx_rtmap.hip).
// The rays of camera sample `sample` for the region of `p`: d_rays double[nrows][nx][6].
hipError_t launch_lens_rays(const KParams& p, int32_t sample, double* d_rays, hipStream_t s);
// One rt_map call per item over p.nrays items (p.cam: monte_carlo_diffusion_times; p.seed): d_rays [n][6],
// d_att [n][3] or null, d_keys int32[n][4], d_paths [n] or null -> d_info int32[n][6], and, each or null,
// d_children [n][2 + pt][9], d_child_paths [n][2 + pt], d_leaves [n][max(n_light, 1)][3].  Nothing goes to p.err.
hipError_t launch_rt_map(KParams p, int mode, const double* d_rays, const double* d_att, const int32_t* d_keys,
                         const uint64_t* d_paths, int32_t* d_info, double* d_children, uint64_t* d_child_paths,
                         double* d_leaves, hipStream_t s);

}  // namespace rtx
