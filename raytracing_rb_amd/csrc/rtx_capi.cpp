// rtx_capi.cpp — the C-ABI of librtx (include/rtx.h): scene/camera upload,
// render entry points, Vec3 helpers.  Host code; kernels in rtx_kernels.hip.
//
// Scene preparation (rtx_scene_build.h) and the camera's restate the
// constructors of the reference (src/world.rb:15-34, src/objects/*.rb,
// src/camera.rb:26-34,129-151) with the same operation order, so every
// constant the device uses has the bits the Ruby code would compute.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <math.h>

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/rtx.h"
#include "rtx_launch.h"
#include "rtx_scene.h"
#include "rtx_scene_build.h"
#include "rtx_vec3.h"

using namespace rtx;

#ifndef RTX_BVH_SAH
#define RTX_BVH_SAH 1                         // default hierarchy splits: 1 binned SAH, 0 median
#endif

constexpr unsigned RTX_WORK_RING = 256;
#ifndef RTX_POSTPONE_NODES
#define RTX_TILE_ORDER_SPHERES 512             // auto tile_order up to this many spheres
#define RTX_POSTPONE_NODES 64                 // hierarchy nodes from which walks are postponed by default
#endif

struct rtx_context {
  int device = 0;
  std::string err;
  // device scene
  std::vector<void*> d_bufs;         // every device allocation of the scene
  SceneDev scene{};
  SceneDev* d_scene = nullptr;
  bool have_scene = false;
  // camera
  CameraDev cam{};
  CameraDev* d_cam = nullptr;
  bool have_cam = false;
  // work buffers
  ErrState* d_err = nullptr;
  unsigned long long* d_counts = nullptr;
  double* d_scratch = nullptr;
  size_t scratch_bytes = 0;
  double* d_stk = nullptr;           // per-lane global ray-stack regions
  size_t stk_bytes = 0;
  double* d_stk2[LV_MAX_PARTS - 1] = {};   // the same for parts 1.. of a multi-stream level render
  size_t stk2_bytes[LV_MAX_PARTS - 1] = {};
  hipStream_t aux[LV_MAX_PARTS - 1] = {};  // bounce levels: the streams of parts 1.. (lv_streams)
  hipEvent_t lv_ev[LV_MAX_PARTS] = {};     // ... after the first batch's reset / after each part
  int* d_work = nullptr;             // ring of per-launch work counters (launches on different streams)
  unsigned work_seq = 0;
  int64_t opt_force_stack = 0;
  int64_t opt_bvh = PlanOpts{}.bvh;               // 0: ordered linear walk; 1: hierarchy from opt_bvh_min spheres; 2: always
  int64_t opt_bvh_sah = RTX_BVH_SAH;  // hierarchy splits: 1 binned SAH, 0 median (applies at the next upload)
  int64_t opt_bvh_min = PlanOpts{}.bvh_min;         // C2 (64 spheres): hierarchy 16.0 ms vs ordered walk 17.8 ms
  int64_t opt_sphere_src = PlanOpts{}.sphere_src;       // 0: LDS staging (measured faster), 1: scalar loads, 2: nodes LDS + leaves global,
                                     // 3: + exact records in LDS, 4: quantized leaves in LDS, -1 auto
  int64_t opt_postpone = -1;         // query_bvh postponing threshold in lanes (-1: auto by hierarchy size)
  int64_t opt_tile_order = -1;       // 1: expensive tiles first (k_tile_cost/k_tile_sort), 0: natural order, -1: auto
  int64_t opt_lds_stack = 0;         // ray-stack entries per lane in LDS (-1: as many as fit; 0 measured fastest)
  int64_t opt_engine = 1;            // 0: persistent lanes (per-lane LIFO ray tree), 1: bounce levels (default: faster, same bits)
  // (the batch options, their defaults and what each one means: rtx_batch.h BatchOpts)
  int64_t opt_lv_batch = BatchOpts{}.lv_batch, opt_lv_stage_pct = BatchOpts{}.lv_stage_pct;
  int64_t opt_lv_rec_pct = BatchOpts{}.lv_rec_pct, opt_lv_floor = BatchOpts{}.lv_floor;
  int64_t opt_lv_split = BatchOpts{}.lv_split, opt_lv_streams = BatchOpts{}.lv_streams;
  int64_t opt_lv_ray_bytes = BatchOpts{}.lv_ray_bytes, opt_lv_hl_cap = BatchOpts{}.lv_hl_cap;
  int64_t opt_lv_sort = BatchOpts{}.lv_sort, opt_lv_sort_from = BatchOpts{}.lv_sort_from;
  int64_t opt_lv_sort_copy = BatchOpts{}.lv_sort_copy;
  int64_t opt_lv_static = -1;        // bounce levels: % of a launch's chunks scheduled statically (-1 auto)
  int64_t opt_lv_round = -1;         // bounce levels: static chunks in rounds of R per workgroup (0 per wave, -1 auto)
  int64_t opt_lv_compact = PlanOpts{}.lv_compact;       // bounce levels: 1 = park hits in an LDS ring and shade full waves, -1 auto (when it fits)
  int64_t opt_lv_grid_div = 1;       // bounce levels: persistent level grids = resident workgroups / this
  int64_t opt_lv_fin_grid = 0;       // bounce levels: tree reduction blocks per CU (grid-stride over tiles), 0 = one block per tile
  int64_t opt_lv_redo_blocks = 8;    // bounce levels: workgroups of the overflow re-render launch (0: all resident)
  int64_t opt_exact_raises = PlanOpts{}.exact_raises;      // 1 (default): local_lights' shadow walks also check the acos raises of the covers they skip
                                     // (§0.0: C2 +3.7 %, C4 +10.4 % against 0)
  int64_t opt_lv_sort_bits = 0;      // bounce levels: 2^bits origin cells per axis (3 or 4); 0 auto: 4 above 512 spheres, else 3
  int64_t opt_lbuf = PlanOpts{}.lbuf;              // bounce levels: 1 = shadow walks through the light buffer where it is staged (§3.18)
  int64_t opt_trace_engine = -1;     // explicit rays: 0 lanes, 1 bounce levels, -1 rtx_trace lanes / rtx_trace_device by batch size
  int64_t last_trace_engine = 0;     // the engine the last trace call ran (read-only option trace_engine_last)
  int n_cus = 0;                     // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  unsigned long long* d_lvstats = nullptr;   // rtx_level_stats of the last bounce-level render call
  int64_t last_sort_levels = 0;              // levels per batch the last bounce-level render binned (lv_sort_last)
  int64_t last_plan = -1;                    // rtx_plan.h pack_plan of its first fused level launch, -1 none (lv_plan_last)
  uint32_t* d_tile_rays = nullptr;   // rtx_tile_rays: rays per 8x8 tile of the last whole-frame level render
  size_t tile_rays_n = 0;
  int32_t* d_rowtiles = nullptr;     // rtx_render_tile_list_device: the tile list on the device
  std::vector<int32_t> rowtiles;     // ... and the list it holds
  size_t rowtiles_cap = 0;
  int64_t opt_kernel_events = 0;     // 1: HIP events around the ray-tree kernel launches (rtx_kernel_time)
  bool err_keys_rays = false;        // the device error keys of the last launch are ray indices (rtx_trace)
  // rtx_render_multi: this context's packed tiles; on the call's first context
  // also the gathered tiles + frame, and the RCCL clique over the call's devices
  double* d_multi = nullptr;
  size_t multi_bytes = 0;
  double* d_gather = nullptr;
  size_t gather_bytes = 0;
  std::vector<int> comm_devs;
  std::vector<ncclComm_t> comms;
  // rtx_kernel_time: event pairs around each ray-tree kernel launch of the last render call
  static constexpr int MAX_EV = 128;
  hipEvent_t ev[2 * MAX_EV] = {};
  int n_ev = 0;
};

static rtx_status fail(rtx_context* c, rtx_status s, const char* fmt, ...) {
  if (c) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    c->err = buf;
  }
  return s;
}

#define HIPCHK(c, expr)                                                                     \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(c, RTX_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

static void free_scene(rtx_context* c) {
  for (void* b : c->d_bufs) (void)hipFree(b);
  c->d_bufs.clear();
  c->have_scene = false;
}

extern "C" {

int32_t rtx_abi_version(void) { return RTX_ABI_VERSION; }

#ifndef RTX_SOURCE_SHA
#define RTX_SOURCE_SHA "unknown"
#endif
const char* rtx_build_id(void) { return RTX_SOURCE_SHA; }

const char* rtx_status_string(rtx_status s) {
  switch (s) {
    case RTX_OK: return "ok";
    case RTX_EZERO_VEC: return "zero vector detected";
    case RTX_ECOLOR_GT1: return "color greater than 1";
    case RTX_EDOMAIN: return "domain error";
    case RTX_EHIP: return "HIP error";
    case RTX_ERCCL: return "RCCL error";
    case RTX_EINVAL: return "invalid argument";
    case RTX_ENOMEM: return "out of memory";
    case RTX_ETYPE: return "TypeError: nil can't be coerced into Integer";
  }
  return "unknown";
}

const char* rtx_last_error(const rtx_context* c) { return c ? c->err.c_str() : "null context"; }

rtx_status rtx_context_create(int32_t device, rtx_context** out) {
  if (!out) return RTX_EINVAL;
  *out = nullptr;
  rtx_context* c = new rtx_context();
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipMalloc(&c->d_err, sizeof(ErrState));
  if (e == hipSuccess) e = hipMalloc(&c->d_counts, sizeof(unsigned long long) * RTX_NCOUNT);
  if (e == hipSuccess) e = hipMalloc(&c->d_scene, sizeof(SceneDev));
  if (e == hipSuccess) e = hipMalloc(&c->d_cam, sizeof(CameraDev));
  if (e == hipSuccess) e = hipMalloc(&c->d_work, sizeof(int) * RTX_WORK_RING);
  if (e == hipSuccess) e = hipMemset(c->d_err, 0, sizeof(unsigned int) * 2);
  if (e == hipSuccess) e = hipMemset(((char*)c->d_err) + 8, 0xFF, sizeof(ErrState) - 8);
  if (e == hipSuccess) {           // keep render_region's stream-ordered buffers pooled between frames
    hipMemPool_t pool;
    if (hipDeviceGetDefaultMemPool(&pool, device) == hipSuccess) {
      uint64_t keep = UINT64_MAX;
      (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
    }
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    fprintf(stderr, "rtx_context_create: %s\n", hipGetErrorString(e));
    delete c;
    return RTX_EHIP;
  }
  *out = c;
  return RTX_OK;
}

void rtx_context_destroy(rtx_context* c) {
  if (!c) return;
  hipSetDevice(c->device);
  free_scene(c);
  hipFree(c->d_err);
  hipFree(c->d_counts);
  hipFree(c->d_scene);
  hipFree(c->d_cam);
  hipFree(c->d_scratch);
  hipFree(c->d_stk);
  for (int j = 0; j < LV_MAX_PARTS - 1; j++) {
    hipFree(c->d_stk2[j]);
    if (c->aux[j]) (void)hipStreamDestroy(c->aux[j]);
  }
  for (hipEvent_t ev : c->lv_ev)
    if (ev) (void)hipEventDestroy(ev);
  hipFree(c->d_work);
  hipFree(c->d_lvstats);
  hipFree(c->d_tile_rays);
  hipFree(c->d_rowtiles);
  hipFree(c->d_multi);
  hipFree(c->d_gather);
  for (size_t k = 0; k < c->comms.size(); k++) {
    hipSetDevice(c->comm_devs[k]);
    ncclCommDestroy(c->comms[k]);
  }
  hipSetDevice(c->device);
  for (hipEvent_t ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  delete c;
}

static bool levels_engine(const rtx_context* c);
static int levels_sph_mode(const rtx_context* c, int split);

static BatchOpts batch_opts(const rtx_context* c) {
  BatchOpts o;
  o.lv_batch = c->opt_lv_batch, o.lv_stage_pct = c->opt_lv_stage_pct, o.lv_rec_pct = c->opt_lv_rec_pct;
  o.lv_floor = c->opt_lv_floor, o.lv_streams = c->opt_lv_streams, o.lv_split = c->opt_lv_split;
  o.lv_hl_cap = c->opt_lv_hl_cap, o.lv_sort = c->opt_lv_sort, o.lv_sort_from = c->opt_lv_sort_from;
  o.lv_sort_copy = c->opt_lv_sort_copy, o.lv_ray_bytes = c->opt_lv_ray_bytes;
  return o;
}

rtx_status rtx_get_option(rtx_context* c, const char* key, int64_t* value) {
  if (!c || !key || !value) return RTX_EINVAL;
  if (!strcmp(key, "engine_effective")) {   // read-only: the engine the next render of this camera runs
    *value = c->have_cam && c->have_scene ? (levels_engine(c) ? 1 : 0) : c->opt_engine;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_sort_last")) {         // read-only: levels per batch the last bounce-level render binned
    *value = c->last_sort_levels;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_plan_last")) {         // read-only: the launch plan of the last bounce-level render's first
    *value = c->last_plan;                    // fused level launch, as the launcher recorded it (-1: none ran)
    return RTX_OK;
  }
  if (!strcmp(key, "trace_engine_last")) {    // read-only: the engine the last rtx_trace / rtx_trace_device call ran
    *value = c->last_trace_engine;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_sort_effective")) {    // read-only: whether the next whole-frame bounce-level render bins its levels
    // the camera samples of a whole-frame render's batch, the frame's tiles split in lv_streams parts
    // (the default two parts give C2 4,147,200 samples per batch, below the 2^22 of sort_from,
    // so a single C2 frame bins nothing; the bench's frames in flight render one part of 8.3 M)
    const BatchOpts o = batch_opts(c);
    *value = c->have_cam && sort_from(c->scene.n_sphere, c->scene.n_light, c->cam.depth,
                                      batch_items((int64_t)((c->cam.width + 7) / 8) * ((c->cam.height + 7) / 8),
                                                  c->cam.pre, c->cam.max_samples, o).n0, o) > 0;
    return RTX_OK;
  }
  if (!strcmp(key, "sph_mode_effective")) {   // read-only: the SphMode of the next bounce-level render's walks
    if (!c->have_scene) return fail(c, RTX_EINVAL, "sph_mode_effective: no scene uploaded");
    *value = resolve_mode(c->scene, levels_sph_mode(c, (int)c->opt_lv_split));
    return RTX_OK;
  }
  if (!strcmp(key, "lv_ray_bytes_effective")) {   // read-only: the staged ray record of the next level render
    *value = c->opt_lv_ray_bytes == 96 || (c->have_cam && !lv_paths32(c->cam.depth, c->cam.pt)) ? 96 : 80;
    return RTX_OK;
  }
  const struct { const char* k; int64_t v; } tab[] = {
      {"engine", c->opt_engine},       {"force_stack", c->opt_force_stack}, {"bvh", c->opt_bvh},
      {"bvh_sah", c->opt_bvh_sah},     {"bvh_min", c->opt_bvh_min},         {"postpone", c->opt_postpone},
      {"lds_stack", c->opt_lds_stack}, {"tile_order", c->opt_tile_order},   {"sphere_src", c->opt_sphere_src},
      {"kernel_events", c->opt_kernel_events}, {"lv_batch", c->opt_lv_batch},
      {"lv_stage_pct", c->opt_lv_stage_pct}, {"lv_rec_pct", c->opt_lv_rec_pct}, {"lv_floor", c->opt_lv_floor},
      {"lv_split", c->opt_lv_split}, {"lv_static", c->opt_lv_static}, {"lv_round", c->opt_lv_round},
      {"lv_compact", c->opt_lv_compact},
      {"lv_streams", c->opt_lv_streams}, {"lv_grid_div", c->opt_lv_grid_div},
      {"lv_redo_blocks", c->opt_lv_redo_blocks},
      {"lv_fin_grid", c->opt_lv_fin_grid}, {"lv_ray_bytes", c->opt_lv_ray_bytes},
      {"exact_raises", c->opt_exact_raises}, {"lv_hl_cap", c->opt_lv_hl_cap}, {"lv_sort", c->opt_lv_sort},
      {"lv_sort_from", c->opt_lv_sort_from}, {"lv_sort_bits", c->opt_lv_sort_bits}, {"lbuf", c->opt_lbuf},
      {"lv_sort_copy", c->opt_lv_sort_copy}, {"trace_engine", c->opt_trace_engine}};
  for (const auto& t : tab)
    if (!strcmp(key, t.k)) {
      *value = t.v;
      return RTX_OK;
    }
  return fail(c, RTX_EINVAL, "unknown option '%s'", key);
}

rtx_status rtx_set_option(rtx_context* c, const char* key, int64_t value) {
  if (!c || !key) return RTX_EINVAL;
  if (!strcmp(key, "engine")) {            // 0: persistent lanes (one ray tree per lane), 1: bounce levels
    if (value < 0 || value > 1) return fail(c, RTX_EINVAL, "engine must be 0 or 1");
    c->opt_engine = value;
    return RTX_OK;
  }
  if (!strcmp(key, "force_stack")) {       // lanes engine: ray-stack entries per lane, rounded up to 8, 16, 32 or 64; 0 auto
    if (value < 0 || value > 64) return fail(c, RTX_EINVAL, "force_stack must be in [0, 64]");
    c->opt_force_stack = value;
    return RTX_OK;
  }
  if (!strcmp(key, "bvh")) {               // 0: linear ordered walk; 1: auto (>= bvh_min spheres); 2: always
    if (value < 0 || value > 2) return fail(c, RTX_EINVAL, "bvh must be 0, 1 or 2");
    c->opt_bvh = value;
    return RTX_OK;
  }
  if (!strcmp(key, "bvh_sah")) {           // hierarchy splits: 1 binned SAH, 0 median (at the next upload)
    c->opt_bvh_sah = value != 0;
    return RTX_OK;
  }
  if (!strcmp(key, "bvh_min")) {           // sphere count from which bvh=1 uses the hierarchy
    if (value < 0) return fail(c, RTX_EINVAL, "bvh_min must be >= 0");
    c->opt_bvh_min = value;
    return RTX_OK;
  }
  if (!strcmp(key, "postpone")) {          // lanes below which hierarchy walks are postponed (-1 auto, 0 never)
    if (value < -1 || value > 64) return fail(c, RTX_EINVAL, "postpone must be in [-1, 64]");
    c->opt_postpone = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lds_stack")) {         // ray-stack entries per lane kept in LDS (-1: as many as fit)
    if (value < -1 || value > 64) return fail(c, RTX_EINVAL, "lds_stack must be in [-1, 64]");
    c->opt_lds_stack = value;
    return RTX_OK;
  }
  if (!strcmp(key, "tile_order")) {        // 1: expensive tiles first; 0: natural (row-major) tile order
    if (value < -1 || value > 1) return fail(c, RTX_EINVAL, "tile_order must be -1, 0 or 1");
    c->opt_tile_order = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_batch")) {          // bounce levels: camera samples per batch
    if (value < 1 || value > (1 << 28)) return fail(c, RTX_EINVAL, "lv_batch must be in [1, 2^28]");
    c->opt_lv_batch = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_stage_pct") || !strcmp(key, "lv_rec_pct")) {   // bounce-level buffer capacities
    if (value < 1 || value > 10000) return fail(c, RTX_EINVAL, "%s must be in [1, 10000]", key);
    (!strcmp(key, "lv_stage_pct") ? c->opt_lv_stage_pct : c->opt_lv_rec_pct) = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_floor")) {          // bounce levels: minimum buffer records (small frames, deep trees)
    if (value < 0 || value > (1 << 26)) return fail(c, RTX_EINVAL, "lv_floor must be in [0, 2^26]");
    c->opt_lv_floor = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_split")) {          // bounce levels: 0 one fused launch per level, 1 trace / shadow / shade
    if (value < 0 || value > 1) return fail(c, RTX_EINVAL, "lv_split must be 0 or 1");
    c->opt_lv_split = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_static")) {         // bounce levels: % of chunks scheduled statically, -1 auto
    if (value < -1 || value > 100) return fail(c, RTX_EINVAL, "lv_static must be in [-1, 100]");
    c->opt_lv_static = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_round")) {          // bounce levels: static chunks in rounds of R per workgroup, 0 per wave, -1 auto
    if (value < -1 || value > LV_ROUND_MAX) return fail(c, RTX_EINVAL, "lv_round must be in [-1, %d]", LV_ROUND_MAX);
    c->opt_lv_round = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_grid_div")) {       // bounce levels: level grids = resident workgroups / this
    if (value < 1 || value > 8) return fail(c, RTX_EINVAL, "lv_grid_div must be in [1, 8]");
    c->opt_lv_grid_div = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_fin_grid")) {       // bounce levels: reduction blocks per CU (grid-stride), 0 = one per tile
    if (value < 0 || value > 64) return fail(c, RTX_EINVAL, "lv_fin_grid must be in [0, 64]");
    c->opt_lv_fin_grid = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_hl_cap")) {         // bounce levels: deferred highlight-check list entries, 0 auto
    if (value < 0 || value > (1 << 26)) return fail(c, RTX_EINVAL, "lv_hl_cap must be in [0, 2^26]");
    c->opt_lv_hl_cap = value;
    return RTX_OK;
  }
  if (!strcmp(key, "exact_raises")) {      // every shadow walk also checks the skipped covers' acos raises
    if (value != 0 && value != 1) return fail(c, RTX_EINVAL, "exact_raises must be 0 or 1");
    c->opt_exact_raises = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_sort")) {           // bounce levels: bin each level's rays before its launch (same bits)
    if (value < -1 || value > 1) return fail(c, RTX_EINVAL, "lv_sort must be -1, 0 or 1");
    c->opt_lv_sort = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_sort_from")) {      // bounce levels: the first level binned (with lv_sort), 0 auto
    if (value < 0 || value > LV_MAXL) return fail(c, RTX_EINVAL, "lv_sort_from must be in [0, %d]", LV_MAXL);
    c->opt_lv_sort_from = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_sort_copy")) {      // bounce levels: binning moves the records into bin order (same bits)
    if (value < 0 || value > 1) return fail(c, RTX_EINVAL, "lv_sort_copy must be 0 or 1");
    c->opt_lv_sort_copy = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_sort_bits")) {      // bounce levels: 2^bits origin cells per axis of a ray bin, 0 auto
    if (value != 0 && value != 3 && value != 4) return fail(c, RTX_EINVAL, "lv_sort_bits must be 0, 3 or 4");
    c->opt_lv_sort_bits = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lbuf")) {              // bounce levels: shadow walks through the light buffer (same bits)
    if (value != 0 && value != 1) return fail(c, RTX_EINVAL, "lbuf must be 0 or 1");
    c->opt_lbuf = value;
    return RTX_OK;
  }
  if (!strcmp(key, "trace_engine")) {      // explicit rays: 0 lanes, 1 bounce levels, -1 auto (rtx_trace_device by batch size)
    if (value < -1 || value > 1) return fail(c, RTX_EINVAL, "trace_engine must be -1, 0 or 1");
    c->opt_trace_engine = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_ray_bytes")) {      // bounce levels: staged ray record size (0 auto)
    if (value != 0 && value != 80 && value != 96) return fail(c, RTX_EINVAL, "lv_ray_bytes must be 0, 80 or 96");
    c->opt_lv_ray_bytes = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_redo_blocks")) {    // bounce levels: overflow re-render grid cap, 0 = all resident
    if (value < 0 || value > (1 << 20)) return fail(c, RTX_EINVAL, "lv_redo_blocks must be in [0, 2^20]");
    c->opt_lv_redo_blocks = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_streams")) {        // bounce levels: tiles in this many interleaved parts on as many streams
    if (value < 1 || value > LV_MAX_PARTS) return fail(c, RTX_EINVAL, "lv_streams must be in [1, %d]", LV_MAX_PARTS);
    c->opt_lv_streams = value;
    return RTX_OK;
  }
  if (!strcmp(key, "lv_compact")) {        // bounce levels: hit compaction in k_level, -1 auto, 2 compact ring
    if (value < -1 || value > 2) return fail(c, RTX_EINVAL, "lv_compact must be -1, 0, 1 or 2");
    c->opt_lv_compact = value;
    return RTX_OK;
  }
  if (!strcmp(key, "kernel_events")) {     // 1: HIP events around the ray-tree launches (rtx_kernel_time)
    c->opt_kernel_events = value != 0;
    return RTX_OK;
  }
  if (!strcmp(key, "sphere_src")) {        // 0: LDS staging; 1: scalar loads; 2: hierarchy nodes in LDS, leaves global;
                                           // 3: + exact records in LDS; 4: quantized leaf records in LDS; -1 auto
    if (value < -1 || value > 4) return fail(c, RTX_EINVAL, "sphere_src must be -1, 0, 1, 2, 3 or 4");
    c->opt_sphere_src = value;
    return RTX_OK;
  }
  return fail(c, RTX_EINVAL, "unknown option '%s'", key);
}

// ------------------------------------------------------------------ scene
// The scene is built on the host first (rtx_scene_build.h): a rejected
// description leaves the previous scene in place.  Then every array goes up.
rtx_status rtx_scene_upload(rtx_context* c, const rtx_scene_desc* sd) {
  if (!c || !sd) return fail(c, RTX_EINVAL, "null argument");
  HostScene H;
  std::string msg;
  hipSetDevice(c->device);
  const rtx_status st = build_host_scene(sd, c->opt_bvh_sah != 0, H, msg);
  if (st != RTX_OK) return fail(c, st, "%s", msg.c_str());
  free_scene(c);
  SceneDev& S = c->scene;
  S = H.dev;
  const Bvh4Builder& bb = *H.bb;
  const struct { const void* src; size_t bytes; const void** dst; bool built; } arrays[] = {
#define RTX_ARRAY(v, member, built) {(v).data(), (v).size() * sizeof((v)[0]), (const void**)&S.member, built}
      RTX_ARRAY(H.runs, runs, true),         RTX_ARRAY(H.sph64, sph64, true),         RTX_ARRAY(H.sph32, sph32, true),
      RTX_ARRAY(H.planes, planes, true),     RTX_ARRAY(H.boxes, boxes, true),         RTX_ARRAY(H.mat, mat, true),
      RTX_ARRAY(bb.nodes, bvh, true),        RTX_ARRAY(bb.slot32, bvh_sph32, true),   RTX_ARRAY(bb.slot64, bvh_sph64, true),
      RTX_ARRAY(H.ql.rec, bvh_q, true),      RTX_ARRAY(bb.slot_obj, bvh_obj, true),   RTX_ARRAY(H.sph_obj, sph_obj, true),
      RTX_ARRAY(H.lights, light, true),      RTX_ARRAY(H.tex, tex, true),             RTX_ARRAY(H.texels, texels, true),
      RTX_ARRAY(H.lb.words, lbuf, H.lb.n != 0), RTX_ARRAY(H.rb.words, rbuf, H.rb.n != 0),
      RTX_ARRAY(H.gates, rgate, H.rb.n != 0)};
#undef RTX_ARRAY
  for (const auto& a : arrays) {
    if (!a.built) continue;                          // (no light or raise buffer: the pointer stays null)
    void* p = nullptr;
    HIPCHK(c, hipMalloc(&p, a.bytes ? a.bytes : 16));
    c->d_bufs.push_back(p);
    if (a.bytes) HIPCHK(c, hipMemcpy(p, a.src, a.bytes, hipMemcpyHostToDevice));
    *a.dst = p;
  }
  HIPCHK(c, hipMemcpy(c->d_scene, &S, sizeof S, hipMemcpyHostToDevice));
  c->have_scene = true;
  return RTX_OK;
}

rtx_status rtx_camera_set(rtx_context* c, const rtx_camera_desc* d) {
  if (!c || !d) return fail(c, RTX_EINVAL, "null argument");
  if (d->width <= 0 || d->height <= 0) return fail(c, RTX_EINVAL, "width/height must be positive");
  if (d->pre_sample_times < 1 || d->pre_sample_times > 16)
    return fail(c, RTX_EINVAL, "pre_sample_times must be in [1, 16]");
  if (d->max_sample_times < 0) return fail(c, RTX_EINVAL, "max_sample_times must be >= 0");
  {
    // device work items are 32-bit: every (8x8-padded) pixel x sample of the frame must fit
    const size_t padded = (size_t)((d->width + 7) / 8) * (size_t)((d->height + 7) / 8) * 64;
    const size_t ms = (size_t)std::max(d->pre_sample_times, d->max_sample_times);
    if (padded * ms > (size_t)INT32_MAX)
      return fail(c, RTX_EINVAL, "%dx%d pixels x %zu samples exceed 2^31 work items", d->width, d->height, ms);
  }
  if (d->trace_depth < 0 || d->trace_depth > 1000) return fail(c, RTX_EINVAL, "bad trace_depth");
  // 0: no path-tracing child at an unlit hit; diffuse_rate / 0.0 (world_object.rb:78) is computed and unused
  if (d->monte_carlo_diffusion_times < 0) return fail(c, RTX_EINVAL, "monte_carlo_diffusion_times must be >= 0");
  uint32_t err = 0;
  CameraDev& k = c->cam;
  memset(&k, 0, sizeof k);
  const V3 pos = v3p(d->position), up = v3p(d->up), front = v3p(d->front);
  const V3 left = vnorm(vcross(up, front), err);                       // camera.rb:130
  set3(k.pos, pos);
  set3(k.left, left);
  set3(k.left_n, vnorm(left, err));                                    // :136
  set3(k.up_n, vnorm(up, err));                                        // :134,136
  set3(k.front, front);
  set3(k.retina_center, vsub(pos, vsc(vnorm(front, err), d->image_distance)));   // :131
  const double od = d->focal_distance * d->image_distance / (d->image_distance - d->focal_distance);  // :139
  set3(k.pofp, vadd(pos, vsc(vnorm(front, err), od)));                // :142
  k.retina_width = d->retina_width;
  k.retina_height = d->retina_height;
  k.aperture_radius = d->aperture_radius;
  k.variant_threshold = d->variant_threshold;
  k.width = d->width;
  k.height = d->height;
  k.pre = d->pre_sample_times;
  k.max_samples = d->max_sample_times;
  k.depth = d->trace_depth;
  k.pt = d->monte_carlo_diffusion_times;
  if (err) return fail(c, RTX_EZERO_VEC, "zero vector detected while building the camera");
  HIPCHK(c, hipMemcpy(c->d_cam, &k, sizeof k, hipMemcpyHostToDevice));
  c->have_cam = true;
  return RTX_OK;
}

// ------------------------------------------------------------------ render
// The lanes engine's ray-stack entries per lane for this camera (8, 16, 32 or 64) into maxs.  A camera
// that needs more than 64, or more than a forced bucket holds, is refused here: a lane never finds its
// stack full (rtx_device.h emit).
static rtx_status required_stack(rtx_context* c, int& maxs) {
  // LIFO depth-first walk: a node at depth d >= 2 pushes <= 2 + pt children.
  const long need = 1 + (long)(c->cam.depth > 1 ? c->cam.depth - 1 : 0) * (1 + (long)c->cam.pt);
  if (need > 64)
    return fail(c, RTX_EINVAL, "trace_depth x monte_carlo_diffusion_times too large: a ray stack of %ld entries, at most 64",
                need);
  maxs = stack_bucket((int)need);
  if (c->opt_force_stack) {
    maxs = stack_bucket((int)c->opt_force_stack);
    if (maxs < need)
      return fail(c, RTX_EINVAL, "force_stack %lld: this camera needs a ray stack of %ld entries",
                  (long long)c->opt_force_stack, need);
  }
  return RTX_OK;
}

// Sphere walk of the next launch (SphMode); the launchers fall back to scalar
// loads when the records exceed the LDS budget.
static int sph_mode(const rtx_context* c) {
  return sph_mode_of(c->scene, (int)c->opt_bvh, (int)c->opt_bvh_min, (int)c->opt_sphere_src);   // (rtx_plan.h)
}

// Global per-lane regions (ray-stack entries beyond LDS) for every lane a persistent launch can keep resident (512 per CU at
// 256 VGPRs; room for 1024).
static rtx_status ensure_stack(rtx_context* c, KParams& p, int maxs) {
  int cus = 0;
  HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  const size_t lanes = (size_t)(cus > 0 ? cus : 1) * 1024;
  const size_t per_lane = (size_t)maxs * 12 * sizeof(double);
  const size_t bytes = lanes * per_lane;
  if (bytes > c->stk_bytes) {
    hipFree(c->d_stk);
    c->d_stk = nullptr;
    c->stk_bytes = 0;
    HIPCHK(c, hipMalloc(&c->d_stk, bytes));
    c->stk_bytes = bytes;
  }
  p.stk_glb = c->d_stk;
  p.stk_glb_lanes = (int32_t)(c->stk_bytes / per_lane);
  return RTX_OK;
}

static rtx_status prep(rtx_context* c, KParams& p, uint64_t seed) {
  // The context's device first: every allocation below and in ensure_stack /
  // ensure_scratch, and every launch, must land on it whatever device the
  // calling thread had selected.
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_scene) return fail(c, RTX_EINVAL, "no scene uploaded");
  if (!c->have_cam) return fail(c, RTX_EINVAL, "no camera set");
  memset(&p, 0, sizeof p);
  p.scene = c->scene;
  p.cam = c->d_cam;
  p.seed = seed;
  p.err = c->d_err;
  p.counts = c->d_counts;
  p.work = c->d_work + (c->work_seq++ % RTX_WORK_RING);
  p.stk_slots_max = c->opt_lds_stack < 0 ? 64 : (int32_t)c->opt_lds_stack;
  p.pre = c->cam.pre;
  p.max_samples = c->cam.max_samples;
  // Postponing long walks pays when walks are long (C4, 341 nodes: 550 -> 507 ms)
  // and costs when they are short (C2, a few nodes: 9.0 -> 9.3 ms).
  p.exact_raises = (int32_t)c->opt_exact_raises;
  p.postpone = c->opt_postpone >= 0 ? (int32_t)c->opt_postpone : (c->scene.n_nodes >= RTX_POSTPONE_NODES ? 16 : 0);
  return RTX_OK;
}

// (al256, the batch arithmetic, lv_paths32 and sort_from: rtx_batch.h)
static int lv_sort_bits(const rtx_context* c) {
  return c->opt_lv_sort_bits ? (int)c->opt_lv_sort_bits : c->scene.n_sphere > 512 ? 4 : 3;
}

// the bounce-level engine's limits: its levels, a ray's child slots, a record's leaves
static bool levels_fit(const rtx_context* c) {
  return c->cam.depth <= LV_MAXL && c->cam.pt + 2 <= 16 && c->scene.n_light <= 255;
}
static bool levels_engine(const rtx_context* c) { return c->opt_engine == 1 && levels_fit(c); }

// ------------------------------------------------------------------ what the launching calls share
// The event pairs around a call's ray-tree kernel launches (option "kernel_events"), created on first use.
static rtx_status kernel_events(rtx_context* c, bool on, KernelEvents& kev) {
  kev = KernelEvents{c->ev, 0, rtx_context::MAX_EV};
  if (on && !c->ev[0])
    for (int k = 0; k < 2 * rtx_context::MAX_EV; k++) HIPCHK(c, hipEventCreate(&c->ev[k]));
  return RTX_OK;
}

// After a call's launches (status e): the pairs it recorded are the context's, and its buffer goes back
// to the pool in stream order whether the launches succeeded or not.
static rtx_status launched(rtx_context* c, hipError_t e, const KernelEvents* kev, void* buf, hipStream_t stream) {
  if (kev) c->n_ev = kev->n;
  const hipError_t f = hipFreeAsync(buf, stream);
  HIPCHK(c, e);
  HIPCHK(c, f);
  return RTX_OK;
}

// The sphere mode of a bounce-level call's walks (before resolve_mode).
// sphere_src auto: C4-sized hierarchies keep their nodes and 16-bit leaf
// records in LDS next to the hit rings (SPH_BVH_QLDS; before round 4 the
// leaves came from global memory, SPH_BVH_MIX, r05b: C4 410 -> 386 ms)
static int levels_sph_mode(const rtx_context* c, int split) {
  return c->opt_sphere_src == -1 ? levels_auto_mode(c->scene, sph_mode(c), (int)c->opt_lv_compact, split) : sph_mode(c);
}

// The layout of a bounce-level call's buffers (rtx_batch.h) for this context's scene, camera and options.
static BatchLayout context_layout(const rtx_context* c, bool trace, bool levels, size_t n0, int parts, size_t npx) {
  return batch_layout(BatchIn{trace, levels, n0, parts, npx, c->scene.n_sphere, c->scene.n_light, c->cam.depth, c->cam.pt},
                      batch_opts(c));
}

// The buffers of one part's set at `base` (rtx_batch.h: a buffer the layout leaves out is a null pointer).
static void carve(KParams& k, char* base, const BatchLayout& L) {
  auto at = [&](BatchBuf b) { return L.present[b] ? base + L.off[b] : nullptr; };
  k.lv_ctl = (LevelCtl*)at(LB_CTL);
  k.lv_redo_of = (int32_t*)at(LB_REDO_OF);
  k.lv_redo_list = (int32_t*)at(LB_REDO_LIST);
  k.lv_redo_smp = (double*)at(LB_REDO_SMP);
  k.lv_stage[0] = (double*)at(LB_STAGE0);
  k.lv_stage[1] = (double*)at(LB_STAGE1);
  k.lv_rec = at(LB_REC);
  k.lv_hit = (double*)at(LB_HIT);
  k.lv_area = (double*)at(LB_AREA);
  k.lv_hlq = (double*)at(LB_HLQ);
  k.lv_key = (uint16_t*)at(LB_KEY);
  k.lv_perm = (uint2*)at(LB_PERM);
  k.lv_bins = (uint32_t*)at(LB_BINS);
  k.lv_sorted = (double*)at(LB_SORTED);
}

// A bounce-level call's buffer (stream-ordered from the device pool like the
// lanes engine's, `parts` sets and the tail) and the level fields of `p` that
// do not depend on which entry the call came through.
static rtx_status level_params(rtx_context* c, KParams& p, const BatchLayout& L, int parts, hipStream_t stream,
                               char*& buf) {
  if (L.refusal) return fail(c, RTX_EINVAL, "%s", L.refusal);
  c->last_sort_levels = L.sort_from > 0 ? std::max(0, c->cam.depth - L.sort_from) : 0;   // (read-only option lv_sort_last)
  c->last_plan = -1;                           // (read-only option lv_plan_last: set by the first fused launch)
  if (!c->d_lvstats) HIPCHK(c, hipMalloc(&c->d_lvstats, sizeof(unsigned long long) * (LV_MAXL + 3)));
  HIPCHK(c, hipMallocAsync((void**)&buf, L.total, stream));
  carve(p, buf, L);
  p.extra_count = (int32_t*)(buf + parts * L.set);   // the tail (the first batch's k_level_begin zeroes the count)
  p.lv_hlq_cap = (uint32_t)L.hlcap;
  p.lv_sort = L.sort_from;
  p.lv_cell_bits = lv_sort_bits(c);
  p.lv_lbuf = (int32_t)c->opt_lbuf;
  p.lv_split = L.split ? 1 : 0;
  p.lv_compact = (int32_t)c->opt_lv_compact;
  p.lv_grid_div = (int32_t)c->opt_lv_grid_div;
  // Static chunks cost no atomics; dynamic claims balance rays of very
  // different cost.  Auto: all static while the sphere records fit one walk
  // workgroup's LDS with room to spare (C2: 5.35 vs 5.9 ms at 50 %), half
  // static for large hierarchies (C4: 437 vs 518 ms all static).
  p.lv_static_pct = c->opt_lv_static >= 0 ? (int32_t)c->opt_lv_static : (c->scene.n_sphere <= 512 ? 100 : 50);
  // The static chunks' owner: a wave (0), or a workgroup whose waves claim them in rounds of R from a
  // counter in LDS.  Auto: R = 8 up to 512 spheres (C2 bench 461.3 -> 497.5 Mpix/s, the
  // 1/8 share 0.703 -> 0.677 ms; 32 ties on the frame and loses on the share, 128 and 512 lose),
  // 32 above (C4 31.53 -> 31.95 Mpix/s; 8: 31.72).
  p.lv_round = c->opt_lv_round >= 0 ? (int32_t)c->opt_lv_round : (c->scene.n_sphere <= 512 ? 8 : 32);
  p.lds_sched = -1;
  p.lv_scap = (uint32_t)L.scap;
  p.lv_slice_log2 = L.slog2;
  p.lv_hslice_log2 = L.hlog2;
  p.lv_lcap = (uint32_t)L.lcap;
  p.lv_rec_bytes = L.rec_bytes;
  p.lv_ray_dbl = L.ray_dbl;
  p.lv_last_level = c->cam.depth >= 1 ? c->cam.depth - 1 : -1;
  p.lv_acc = c->d_lvstats;
  p.samples = nullptr;
  return RTX_OK;
}

// render_region for the bounce-level engine: batches of
// 8x8 tiles, one launch per tree level, the trees reduced by k_tree_finalize.
// Buffers for one batch: staging (2 x lv_stage_pct % of the batch items x
// 96 B), tree records (lv_rec_pct % x 32 B with one light), the re-render list.
static rtx_status render_levels(rtx_context* c, KParams& p, int maxs, hipStream_t stream) {
  const BatchItems it = batch_items(((p.nx + 7) / 8) * ((p.nrows + 7) / 8), p.pre, p.max_samples, batch_opts(c));
  // One buffer set per part: with lv_streams = P the region's tiles are
  // rendered in P interleaved parts at once, parts 1.. on the context's aux
  // streams (one part's level tails, launch gaps and reductions overlap the
  // others' levels).  The extra-sample list and the statistics are shared
  // (appended / added atomically); each part has its own level buffers, its
  // own lanes-engine work counter and ray stacks for its overflow re-render.
  const int parts = it.parts;
  const BatchLayout L = context_layout(c, false, true, it.n0, parts, (size_t)p.nx * p.nrows);
  char* buf = nullptr;
  if (rtx_status s = level_params(c, p, L, parts, stream, buf)) return s;
  p.extra_list = p.extra_count + 64;
  p.lv_redo_blocks = (int32_t)c->opt_lv_redo_blocks;
  p.lv_fin_tiles = (int32_t)c->opt_lv_fin_grid;   // (blocks per CU here; the launcher sets the tile count)
  LvAux aux{};
  if (parts > 1) {
    aux.parts = parts;
    for (hipEvent_t& ev : c->lv_ev)
      if (!ev) HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    aux.ev_first = c->lv_ev[0];
    const size_t stk = (size_t)p.stk_glb_lanes * (size_t)maxs * 12 * sizeof(double);
    for (int j = 0; j < parts - 1; j++) {
      if (!c->aux[j]) HIPCHK(c, hipStreamCreateWithFlags(&c->aux[j], hipStreamNonBlocking));
      if (stk > c->stk2_bytes[j]) {
        hipFree(c->d_stk2[j]);
        c->d_stk2[j] = nullptr;
        c->stk2_bytes[j] = 0;
        HIPCHK(c, hipMalloc(&c->d_stk2[j], stk));
        c->stk2_bytes[j] = stk;
      }
      KParams& q = aux.pb[j];
      q = p;
      carve(q, buf + (size_t)(j + 1) * L.set, L);
      q.work = reinterpret_cast<int*>(&q.lv_ctl->pad[0]);   // zeroed by its part's k_level_begin
      q.stk_glb = c->d_stk2[j];
      aux.s2[j] = c->aux[j];
      aux.ev_done[j] = c->lv_ev[j + 1];
    }
  }
  KernelEvents kev;
  if (rtx_status s = kernel_events(c, c->opt_kernel_events != 0, kev)) return s;
  KernelEvents* const ke = c->opt_kernel_events ? &kev : nullptr;
  const hipError_t e = launch_levels(p, levels_sph_mode(c, (int)c->opt_lv_split), maxs, std::max(1, c->cam.depth),
                                     it.batch_tiles, stream, ke, parts > 1 ? &aux : nullptr, &c->last_plan);
  return launched(c, e, ke, buf, stream);
}

// launch_render with its per-launch sample records and extra-sample list,
// allocated stream-ordered (the device's default pool keeps the memory, so
// after the first frame this costs no hipMalloc) and freed after the launch,
// so launches of one context on different streams never share them.
static rtx_status render_region(rtx_context* c, KParams& p, bool count, int maxs, hipStream_t stream) {
  const size_t npx = (size_t)p.nx * p.nrows;
  if (npx == 0) return RTX_OK;
  if (!count && levels_engine(c)) {
    const size_t padded = (size_t)((p.nx + 7) / 8) * ((p.nrows + 7) / 8) * 64;
    if (padded * (size_t)std::max(p.pre, p.max_samples) > (size_t)INT32_MAX)
      return fail(c, RTX_EINVAL, "%zu pixels x samples exceed the 2^31 work items of one launch", npx);
    return render_levels(c, p, maxs, stream);
  }
  const size_t ms = (size_t)std::max(p.pre, p.max_samples);
  // Work items are 32-bit on the device: (8x8-padded pixels) x samples must fit.
  const size_t padded = (size_t)((p.nx + 7) / 8) * ((p.nrows + 7) / 8) * 64;
  if (padded * ms > (size_t)INT32_MAX)
    return fail(c, RTX_EINVAL, "%zu pixels x %zu samples exceed the 2^31 work items of one launch", npx, ms);
  const size_t smp_bytes = npx * ms * 4 * sizeof(double);
  void* buf = nullptr;
  const size_t tiles = (size_t)((p.nx + 7) / 8) * ((p.nrows + 7) / 8);
  HIPCHK(c, hipMallocAsync(&buf, smp_bytes + (npx + 64 + 2 * tiles) * sizeof(int32_t), stream));
  p.samples = (double*)buf;
  p.extra_count = (int32_t*)((char*)buf + smp_bytes);
  p.extra_list = p.extra_count + 64;
  p.tile_cls = p.extra_list + npx;
  // Auto: the probe is an ordered linear walk, cheap for a few hundred spheres
  // (C2: 9.2 -> 8.9 ms); on C4 (4,096 spheres) it costs 2.2 ms and the order
  // gains nothing (the frame is 500 ms of evenly expensive tiles).
  const bool order = c->opt_tile_order > 0 || (c->opt_tile_order < 0 && c->scene.n_sphere <= RTX_TILE_ORDER_SPHERES);
  p.tile_order = order ? p.tile_cls + tiles : nullptr;
  KernelEvents kev;
  if (rtx_status s = kernel_events(c, c->opt_kernel_events && !count, kev)) return s;
  KernelEvents* const ke = c->opt_kernel_events && !count ? &kev : nullptr;
  return launched(c, launch_render(p, sph_mode(c), count, maxs, stream, ke), ke, buf, stream);
}

rtx_status rtx_render_device(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint64_t seed,
                             double* d_out, size_t row_stride, void* stream) {
  if (!c) return RTX_EINVAL;
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  if (x0 < 0 || y0 < 0 || x1 > c->cam.width || y1 > c->cam.height || x0 > x1 || y0 > y1)
    return fail(c, RTX_EINVAL, "region [%d,%d)x[%d,%d) outside the %dx%d image", x0, x1, y0, y1,
                c->cam.width, c->cam.height);
  if (row_stride < (size_t)(x1 - x0) * 3) return fail(c, RTX_EINVAL, "row_stride too small");
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  hipSetDevice(c->device);
  p.x0 = x0;
  p.nx = x1 - x0;
  p.y0 = y0;
  p.nrows = y1 - y0;
  p.out = d_out;
  p.stride = row_stride;
  if (x0 == 0 && y0 == 0 && x1 == c->cam.width && y1 == c->cam.height && levels_engine(c)) {
    // the whole frame: the reduction records rays per 8x8 tile (rtx_tile_rays)
    const size_t nt = (size_t)((x1 + 7) / 8) * ((y1 + 7) / 8);
    if (nt > c->tile_rays_n) {
      hipFree(c->d_tile_rays);
      c->d_tile_rays = nullptr;
      c->tile_rays_n = 0;
      HIPCHK(c, hipMalloc(&c->d_tile_rays, nt * sizeof(uint32_t)));
      HIPCHK(c, hipMemset(c->d_tile_rays, 0, nt * sizeof(uint32_t)));
      c->tile_rays_n = nt;
    }
    p.tile_rays = c->d_tile_rays;
  }
  return render_region(c, p, false, maxs, (hipStream_t)stream);
}

rtx_status rtx_tile_rays(rtx_context* c, int64_t* out, int32_t n) {
  if (!c || (!out && n > 0) || n < 0) return fail(c, RTX_EINVAL, "bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<uint32_t> v(c->tile_rays_n);
  if (c->d_tile_rays) {
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(v.data(), c->d_tile_rays, v.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  for (int k = 0; k < n; k++) out[k] = (size_t)k < v.size() ? (int64_t)v[k] : 0;
  return RTX_OK;
}

rtx_status rtx_render_tile_list_device(rtx_context* c, const int32_t* tiles, int32_t n, int32_t tile_rows,
                                       uint64_t seed, double* d_packed, void* stream) {
  if (!c) return RTX_EINVAL;
  if (n < 0 || (n > 0 && (!tiles || !d_packed)) || tile_rows <= 0) return fail(c, RTX_EINVAL, "bad tile list");
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  if (n == 0) return RTX_OK;
  const int ntiles = (c->cam.height + tile_rows - 1) / tile_rows;
  if ((int64_t)n * tile_rows > INT32_MAX) return fail(c, RTX_EINVAL, "%d tiles of %d rows exceed 2^31 rows", n, tile_rows);
  // an index past the bottom is padding: clamped to ntiles (rows y >= height render nothing), so no
  // tile * tile_rows product can overflow on the device (row_to_y)
  std::vector<int32_t> list(tiles, tiles + n);
  for (int k = 0; k < n; k++) {
    if (list[k] < 0) return fail(c, RTX_EINVAL, "tile %d: negative index %d", k, list[k]);
    if (list[k] > ntiles) list[k] = ntiles;
  }
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  hipSetDevice(c->device);
  if (c->rowtiles != list) {
    if ((size_t)n > c->rowtiles_cap) {
      hipFree(c->d_rowtiles);
      c->d_rowtiles = nullptr;
      c->rowtiles_cap = 0;
      HIPCHK(c, hipMalloc(&c->d_rowtiles, (size_t)n * sizeof(int32_t)));
      c->rowtiles_cap = (size_t)n;
    }
    c->rowtiles = list;
    // ordered before this call's launches on `stream` (a caller that changes
    // the list while another stream's render still reads it must sync first)
    HIPCHK(c, hipMemcpyAsync(c->d_rowtiles, c->rowtiles.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice,
                             (hipStream_t)stream));
  }
  p.x0 = 0;
  p.nx = c->cam.width;
  p.nrows = n * tile_rows;
  p.tile_rows = tile_rows;
  p.rank = 0;
  p.nranks = 1;
  p.row_tiles = c->d_rowtiles;
  p.out = d_packed;
  p.stride = (size_t)c->cam.width * 3;
  return render_region(c, p, false, maxs, (hipStream_t)stream);
}

int32_t rtx_tiles_rows_per_rank(int32_t height, int32_t tile_rows, int32_t nranks) {
  if (tile_rows <= 0 || nranks <= 0) return 0;
  const int32_t tiles = (height + tile_rows - 1) / tile_rows;
  return ((tiles + nranks - 1) / nranks) * tile_rows;
}

rtx_status rtx_render_tiles_device(rtx_context* c, int32_t tile_rows, int32_t rank, int32_t nranks,
                                   uint64_t seed, double* d_packed, void* stream) {
  if (!c) return RTX_EINVAL;
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  if (tile_rows <= 0 || nranks <= 0 || rank < 0 || rank >= nranks) return fail(c, RTX_EINVAL, "bad tiling");
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  hipSetDevice(c->device);
  p.x0 = 0;
  p.nx = c->cam.width;
  p.nrows = rtx_tiles_rows_per_rank(c->cam.height, tile_rows, nranks);
  p.tile_rows = tile_rows;
  p.rank = rank;
  p.nranks = nranks;
  p.out = d_packed;
  p.stride = (size_t)c->cam.width * 3;
  return render_region(c, p, false, maxs, (hipStream_t)stream);
}

rtx_status rtx_level_stats(rtx_context* c, int64_t* out, int32_t n) {
  if (!c || !out || n < 0) return fail(c, RTX_EINVAL, "bad arguments");
  HIPCHK(c, hipSetDevice(c->device));
  unsigned long long v[LV_MAXL + 3] = {0};
  if (c->d_lvstats) {
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(v, c->d_lvstats, sizeof v, hipMemcpyDeviceToHost));
  }
  for (int k = 0; k < n; k++) out[k] = k < LV_MAXL + 3 ? (int64_t)v[k] : 0;
  return RTX_OK;
}

rtx_status rtx_kernel_time(rtx_context* c, double* total_ms, int32_t* launches) {
  if (!c || !total_ms) return fail(c, RTX_EINVAL, "null argument");
  HIPCHK(c, hipSetDevice(c->device));
  // The union of the launches' intervals (the parts of a multi-stream
  // level render overlap), each placed relative to the first launch's start.
  std::vector<std::pair<double, double>> iv;
  for (int k = 0; k < c->n_ev; k++) {
    float a = 0.0f, b = 0.0f;
    HIPCHK(c, hipEventSynchronize(c->ev[2 * k + 1]));
    HIPCHK(c, hipEventElapsedTime(&a, c->ev[0], c->ev[2 * k]));
    HIPCHK(c, hipEventElapsedTime(&b, c->ev[0], c->ev[2 * k + 1]));
    iv.emplace_back(a, b);
  }
  std::sort(iv.begin(), iv.end());
  double sum = 0.0, lo = 0.0, hi = -1e300;
  for (const auto& v : iv) {
    if (v.first > hi) {
      if (hi > lo) sum += hi - lo;
      lo = v.first;
      hi = v.second;
    } else if (v.second > hi) {
      hi = v.second;
    }
  }
  if (hi > lo) sum += hi - lo;
  *total_ms = sum;
  if (launches) *launches = c->n_ev;
  return RTX_OK;
}

// Waits for `stream`, moves the device's raise record into `e` and resets it.
static rtx_status take_errors(rtx_context* c, void* stream, ErrState* e) {
  hipSetDevice(c->device);
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  HIPCHK(c, hipMemcpy(e, c->d_err, sizeof *e, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemset(c->d_err, 0, 8));
  HIPCHK(c, hipMemset(((char*)c->d_err) + 8, 0xFF, sizeof(ErrState) - 8));
  HIPCHK(c, hipDeviceSynchronize());
  return RTX_OK;
}

// The first raise the reference would meet: the smallest key over the codes.
static rtx_status report_errors(rtx_context* c, const ErrState& e) {
  if (!e.flags) return RTX_OK;
  // device ERR_ code -> rtx_status (index = ERR_ code, rtx_vec3.h)
  static const rtx_status status_of[5] = {RTX_OK, RTX_EZERO_VEC, RTX_ECOLOR_GT1, RTX_EDOMAIN, RTX_ETYPE};
  rtx_status first = RTX_OK;
  unsigned long long key = ~0ull;
  for (int code = 1; code < 5; code++)
    if ((e.flags >> code & 1) && e.first[code] < key) {
      key = e.first[code];
      first = status_of[code];
    }
  const char* more = __builtin_popcount(e.flags) > 1 ? " (and other errors)" : "";
  if (c->err_keys_rays) return fail(c, first, "%s at ray %llu%s", rtx_status_string(first), key, more);
  // pixel keys are (x * height + y) * 2 + phase: render_sync's x-outer, y-inner
  // order (camera.rb:102-103), pre samples before extra samples (px_key)
  const unsigned long long H = c->have_cam ? (unsigned long long)c->cam.height : 1;
  const unsigned long long pix = key >> 1;
  return fail(c, first, "%s at pixel (%llu,%llu)%s", rtx_status_string(first), pix / H, pix % H, more);
}

rtx_status rtx_sync(rtx_context* c, void* stream) {
  if (!c) return RTX_EINVAL;
  ErrState e;
  const rtx_status s = take_errors(c, stream, &e);
  if (s) return s;
  return report_errors(c, e);
}

static rtx_status ensure_scratch(rtx_context* c, size_t bytes) {
  if (bytes <= c->scratch_bytes) return RTX_OK;
  hipFree(c->d_scratch);
  c->d_scratch = nullptr;
  c->scratch_bytes = 0;
  HIPCHK(c, hipMalloc(&c->d_scratch, bytes));
  c->scratch_bytes = bytes;
  return RTX_OK;
}

rtx_status rtx_render(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint64_t seed,
                      double* out, size_t row_stride) {
  if (!c || !out) return fail(c, RTX_EINVAL, "null argument");
  const int w = x1 - x0, h = y1 - y0;
  if (w < 0 || h < 0) return fail(c, RTX_EINVAL, "empty region");
  if (row_stride < (size_t)w * 3) return fail(c, RTX_EINVAL, "row_stride too small");
  if (w == 0 || h == 0) return RTX_OK;
  rtx_status s = rtx_sync(c, nullptr);               // clear stale device errors
  (void)s;
  hipSetDevice(c->device);
  if ((s = ensure_scratch(c, sizeof(double) * 3 * (size_t)w * h))) return s;
  if ((s = rtx_render_device(c, x0, y0, x1, y1, seed, c->d_scratch, (size_t)w * 3, nullptr))) return s;
  HIPCHK(c, hipMemcpy2D(out, row_stride * sizeof(double), c->d_scratch, (size_t)w * 3 * sizeof(double),
                        (size_t)w * 3 * sizeof(double), h, hipMemcpyDeviceToHost));
  return rtx_sync(c, nullptr);
}

rtx_status rtx_render_tiles(rtx_context* c, int32_t tile_rows, int32_t rank, int32_t nranks, uint64_t seed,
                            double* packed) {
  if (!c || !packed) return fail(c, RTX_EINVAL, "null argument");
  if (!c->have_cam) return fail(c, RTX_EINVAL, "no camera set");
  if (tile_rows <= 0 || nranks <= 0 || rank < 0 || rank >= nranks) return fail(c, RTX_EINVAL, "bad tiling");
  rtx_status s = rtx_sync(c, nullptr);               // clear stale device errors
  (void)s;
  hipSetDevice(c->device);
  const size_t rows = (size_t)rtx_tiles_rows_per_rank(c->cam.height, tile_rows, nranks);
  const size_t bytes = sizeof(double) * 3 * rows * (size_t)c->cam.width;
  if (bytes == 0) return RTX_OK;
  if ((s = ensure_scratch(c, bytes))) return s;
  HIPCHK(c, hipMemset(c->d_scratch, 0, bytes));
  if ((s = rtx_render_tiles_device(c, tile_rows, rank, nranks, seed, c->d_scratch, nullptr))) return s;
  HIPCHK(c, hipMemcpy(packed, c->d_scratch, bytes, hipMemcpyDeviceToHost));
  return rtx_sync(c, nullptr);
}

static rtx_status grow(rtx_context* c, double** buf, size_t* cap, size_t bytes) {
  if (bytes <= *cap) return RTX_OK;
  hipFree(*buf);
  *buf = nullptr;
  *cap = 0;
  HIPCHK(c, hipMalloc((void**)buf, bytes));
  *cap = bytes;
  return RTX_OK;
}

// rtx_render_multi / rtx_render_multi_plan: plan == nullptr deals the tiles
// round-robin, else rank k renders the list plan[k * per_rank .. + per_rank).
static rtx_status render_multi(rtx_context* const* ctxs, int32_t n, int32_t tile_rows, const int32_t* plan,
                               int32_t per_rank, uint64_t seed, double* out, size_t row_stride) {
  if (!ctxs || n < 1 || !ctxs[0]) return RTX_EINVAL;
  rtx_context* c0 = ctxs[0];
  if (!out || tile_rows <= 0) return fail(c0, RTX_EINVAL, "bad arguments");
  if (plan && (per_rank < 1 || (int64_t)per_rank * tile_rows > INT32_MAX / 2))
    return fail(c0, RTX_EINVAL, "bad plan: %d tiles per rank", per_rank);
  std::vector<int> devs(n);
  for (int k = 0; k < n; k++) {
    rtx_context* c = ctxs[k];
    if (!c || !c->have_scene || !c->have_cam) return fail(c0, RTX_EINVAL, "context %d has no scene or camera", k);
    if (c->cam.width != c0->cam.width || c->cam.height != c0->cam.height)
      return fail(c0, RTX_EINVAL, "context %d renders a different image size", k);
    devs[k] = c->device;
  }
  const int W = c0->cam.width, H = c0->cam.height;
  if (row_stride < (size_t)W * 3) return fail(c0, RTX_EINVAL, "row_stride too small");
  const int ntiles = (H + tile_rows - 1) / tile_rows;
  std::vector<int32_t> pl;                                     // the plan, padding clamped to ntiles
  if (plan) {
    pl.assign(plan, plan + (size_t)n * per_rank);
    std::vector<char> seen(ntiles, 0);
    for (int32_t& t : pl) {
      if (t < 0) return fail(c0, RTX_EINVAL, "plan: negative tile index %d", t);
      if (t >= ntiles) {
        t = ntiles;
        continue;
      }
      if (seen[t]++) return fail(c0, RTX_EINVAL, "plan: tile %d listed twice", t);
    }
    for (int t = 0; t < ntiles; t++)
      if (!seen[t]) return fail(c0, RTX_EINVAL, "plan: tile %d in no rank's list", t);
  }
  const int R = plan ? per_rank * tile_rows : rtx_tiles_rows_per_rank(H, tile_rows, n);
  const size_t count = (size_t)R * W * 3;                      // doubles per rank
  // clear stale device errors (as rtx_render: unsynced raises of earlier
  // asynchronous calls on these contexts are discarded, include/rtx.h)
  for (int k = 0; k < n; k++) (void)rtx_sync(ctxs[k], nullptr);
  // every rank renders its tiles on its own device; the devices run concurrently
  for (int k = 0; k < n; k++) {
    rtx_context* c = ctxs[k];
    HIPCHK(c0, hipSetDevice(c->device));
    rtx_status s = grow(c, &c->d_multi, &c->multi_bytes, count * sizeof(double));
    if (!s)
      s = plan ? rtx_render_tile_list_device(c, pl.data() + (size_t)k * per_rank, per_rank, tile_rows, seed,
                                             c->d_multi, nullptr)
               : rtx_render_tiles_device(c, tile_rows, k, n, seed, c->d_multi, nullptr);
    if (s) return fail(c0, s, "rank %d: %s", k, rtx_last_error(c));
  }
  HIPCHK(c0, hipSetDevice(c0->device));
  const size_t plan_dbl = plan ? ((size_t)n * per_rank * sizeof(int32_t) + 7) / 8 : 0;
  rtx_status s = grow(c0, &c0->d_gather, &c0->gather_bytes,
                      ((size_t)n * count + (size_t)W * H * 3 + plan_dbl) * sizeof(double));
  if (s) return s;
  double* gathered = c0->d_gather;
  double* frame = c0->d_gather + (size_t)n * count;
  int32_t* d_plan = plan ? reinterpret_cast<int32_t*>(frame + (size_t)W * H * 3) : nullptr;
  if (plan) HIPCHK(c0, hipMemcpy(d_plan, pl.data(), pl.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  bool distinct = true;
  for (int a = 0; a < n; a++)
    for (int b = a + 1; b < n; b++) distinct = distinct && devs[a] != devs[b];
  if (distinct) {
    // ONE gather to rank 0 over RCCL (xGMI): grouped ncclSend / ncclRecv on
    // every device's stream, ordered after that device's render.
    if (c0->comm_devs != devs) {
      for (size_t k = 0; k < c0->comms.size(); k++) {
        hipSetDevice(c0->comm_devs[k]);
        ncclCommDestroy(c0->comms[k]);
      }
      c0->comms.assign(n, nullptr);
      c0->comm_devs.clear();
      const ncclResult_t ri = ncclCommInitAll(c0->comms.data(), n, devs.data());
      if (ri != ncclSuccess) {
        c0->comms.clear();                       // nothing to destroy later
        return fail(c0, RTX_ERCCL, "ncclCommInitAll: %s", ncclGetErrorString(ri));
      }
      c0->comm_devs = devs;
    }
    // Every call between GroupStart and GroupEnd is made and GroupEnd always
    // runs, so a failure never leaves this thread inside an open RCCL group;
    // after one the cached communicators are torn down (the next call
    // re-initialises them).
    ncclResult_t r = ncclGroupStart();
    const char* what = r != ncclSuccess ? "ncclGroupStart" : nullptr;
    if (r == ncclSuccess) {
      for (int k = 0; k < n; k++) {
        hipSetDevice(devs[k]);
        const ncclResult_t rk = ncclSend(ctxs[k]->d_multi, count, ncclFloat64, 0, c0->comms[k], nullptr);
        if (rk != ncclSuccess && !what) r = rk, what = "ncclSend";
      }
      hipSetDevice(devs[0]);
      for (int k = 0; k < n; k++) {
        const ncclResult_t rk = ncclRecv(gathered + (size_t)k * count, count, ncclFloat64, k, c0->comms[0], nullptr);
        if (rk != ncclSuccess && !what) r = rk, what = "ncclRecv";
      }
      const ncclResult_t re = ncclGroupEnd();
      if (re != ncclSuccess && !what) r = re, what = "ncclGroupEnd";
    }
    if (what) {
      // sends / receives may already be enqueued: abort (ncclCommDestroy would
      // wait for them and can hang where abort does not)
      for (size_t k = 0; k < c0->comms.size(); k++) {
        hipSetDevice(c0->comm_devs[k]);
        ncclCommAbort(c0->comms[k]);
      }
      c0->comms.clear();
      c0->comm_devs.clear();
      hipSetDevice(devs[0]);
      return fail(c0, RTX_ERCCL, "%s: %s", what, ncclGetErrorString(r));
    }
  } else {
    // several ranks on one device (more workers than GPUs): device copies
    for (int k = 0; k < n; k++) {
      HIPCHK(c0, hipSetDevice(devs[k]));
      HIPCHK(c0, hipDeviceSynchronize());
      HIPCHK(c0, hipMemcpyPeer(gathered + (size_t)k * count, devs[0], ctxs[k]->d_multi, devs[k],
                               count * sizeof(double)));
    }
  }
  HIPCHK(c0, hipSetDevice(devs[0]));
  HIPCHK(c0, plan ? launch_unpack_plan(gathered, W, H, tile_rows, n, per_rank, d_plan, frame, (size_t)W * 3, nullptr)
                  : launch_unpack(gathered, W, H, tile_rows, n, R, frame, (size_t)W * 3, nullptr));
  HIPCHK(c0, hipMemcpy2D(out, row_stride * sizeof(double), frame, (size_t)W * 3 * sizeof(double),
                         (size_t)W * 3 * sizeof(double), H, hipMemcpyDeviceToHost));
  // the ranks' reference raises, merged: the first in render_sync order over
  // the whole frame (pixel keys do not depend on the rank that rendered them)
  ErrState all;
  all.flags = 0;
  for (int code = 0; code < 5; code++) all.first[code] = ~0ull;
  // Every rank's record is taken (and reset) even after one fails, so no
  // rank is left holding raises for a later call; the first failure wins.
  rtx_status take_fail = RTX_OK;
  int fail_rank = -1;
  for (int k = 0; k < n; k++) {
    ErrState e;
    const rtx_status st = take_errors(ctxs[k], nullptr, &e);
    if (st) {
      if (!take_fail) take_fail = st, fail_rank = k;
      continue;
    }
    all.flags |= e.flags;
    for (int code = 0; code < 5; code++)
      if (e.first[code] < all.first[code]) all.first[code] = e.first[code];
  }
  hipSetDevice(devs[0]);
  if (take_fail) return fail(c0, take_fail, "rank %d: %s", fail_rank, rtx_last_error(ctxs[fail_rank]));
  return report_errors(c0, all);
}

int32_t rtx_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

rtx_status rtx_render_multi(rtx_context* const* ctxs, int32_t n, int32_t tile_rows, uint64_t seed, double* out,
                            size_t row_stride) {
  return render_multi(ctxs, n, tile_rows, nullptr, 0, seed, out, row_stride);
}

rtx_status rtx_render_multi_plan(rtx_context* const* ctxs, int32_t n, int32_t tile_rows, const int32_t* plan,
                                 int32_t per_rank, uint64_t seed, double* out, size_t row_stride) {
  if (!plan) return ctxs && n > 0 && ctxs[0] ? fail(ctxs[0], RTX_EINVAL, "null plan") : RTX_EINVAL;
  return render_multi(ctxs, n, tile_rows, plan, per_rank, seed, out, row_stride);
}

rtx_status rtx_tile_probe(rtx_context* c, int64_t* out, int32_t n) {
  if (!c || n < 0 || (n > 0 && !out)) return fail(c, RTX_EINVAL, "bad arguments");
  KParams p;
  rtx_status s = prep(c, p, 1);
  if (s) return s;
  HIPCHK(c, hipSetDevice(c->device));
  p.x0 = 0;
  p.nx = c->cam.width;
  p.y0 = 0;
  p.nrows = c->cam.height;
  p.tile_rows = 0;
  const int tiles = ((p.nx + 7) / 8) * ((p.nrows + 7) / 8);
  int32_t* d = nullptr;
  HIPCHK(c, hipMalloc(&d, (size_t)std::max(1, tiles) * sizeof(int32_t)));
  std::vector<int32_t> v(tiles);
  hipError_t e = launch_tile_probe(p, d, nullptr);
  if (e == hipSuccess) e = hipMemcpy(v.data(), d, (size_t)tiles * sizeof(int32_t), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  HIPCHK(c, e);
  for (int k = 0; k < n; k++) out[k] = k < tiles ? (int64_t)v[k] : 0;
  return RTX_OK;
}

// First-hit feature buffers (rtx_aov.hip).  Like rtx_tile_probe the pass
// records no raise: the device's raise record and rtx_sync's state stay as
// they are.
rtx_status rtx_first_hit_device(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint64_t seed,
                                int32_t sample, int32_t* d_ids, double* d_geom, void* stream) {
  if (!c) return RTX_EINVAL;
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  if (x0 < 0 || y0 < 0 || x1 > c->cam.width || y1 > c->cam.height || x0 >= x1 || y0 >= y1)
    return fail(c, RTX_EINVAL, "region [%d,%d)x[%d,%d) empty or outside the %dx%d image", x0, x1, y0, y1,
                c->cam.width, c->cam.height);
  const int ms = std::max(c->cam.pre, c->cam.max_samples);
  if (sample < 0 || sample >= ms) return fail(c, RTX_EINVAL, "sample %d outside [0, %d)", sample, ms);
  if (!d_ids && !d_geom) return fail(c, RTX_EINVAL, "both output buffers are null");
  p.x0 = x0;
  p.nx = x1 - x0;
  p.y0 = y0;
  p.nrows = y1 - y0;
  HIPCHK(c, launch_first_hit(p, sph_mode(c), sample, d_ids, d_geom, (hipStream_t)stream));
  return RTX_OK;
}

rtx_status rtx_first_hit(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint64_t seed,
                         int32_t sample, int32_t* ids, double* geom) {
  if (!c) return RTX_EINVAL;
  if (!ids && !geom) return fail(c, RTX_EINVAL, "both output buffers are null");
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  if (x0 < 0 || y0 < 0 || x1 > c->cam.width || y1 > c->cam.height || x0 >= x1 || y0 >= y1)
    return fail(c, RTX_EINVAL, "region [%d,%d)x[%d,%d) empty or outside the %dx%d image", x0, x1, y0, y1,
                c->cam.width, c->cam.height);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t n = (size_t)(x1 - x0) * (size_t)(y1 - y0);
  const size_t geom_bytes = geom ? n * 10 * sizeof(double) : 0, ids_bytes = ids ? n * 3 * sizeof(int32_t) : 0;
  rtx_status s = ensure_scratch(c, geom_bytes + ids_bytes);
  if (s) return s;
  double* d_geom = geom ? c->d_scratch : nullptr;
  int32_t* d_ids = ids ? reinterpret_cast<int32_t*>(reinterpret_cast<char*>(c->d_scratch) + geom_bytes) : nullptr;
  if ((s = rtx_first_hit_device(c, x0, y0, x1, y1, seed, sample, d_ids, d_geom, nullptr))) return s;
  // (stream-ordered blocking copies: no rtx_sync, whose raise record this pass leaves alone)
  if (geom) HIPCHK(c, hipMemcpy(geom, d_geom, geom_bytes, hipMemcpyDeviceToHost));
  if (ids) HIPCHK(c, hipMemcpy(ids, d_ids, ids_bytes, hipMemcpyDeviceToHost));
  return RTX_OK;
}

// Batched World queries (rtx_aov.hip k_intersect, rtx_query.hip k_lit_area).
// They need the scene only: prep() would demand a camera the kernels never
// read.  Nothing is recorded in the device's raise record.
static rtx_status prep_query(rtx_context* c, KParams& p, int32_t n) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_scene) return fail(c, RTX_EINVAL, "no scene uploaded");
  memset(&p, 0, sizeof p);
  p.scene = c->scene;
  p.nrays = n;
  p.exact_raises = (int32_t)c->opt_exact_raises;
  return RTX_OK;
}

rtx_status rtx_intersect_device(rtx_context* c, int32_t n, const double* d_rays, int32_t* d_ids, double* d_geom,
                                void* stream) {
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative ray count");
  if (!c->have_scene) return fail(c, RTX_EINVAL, "no scene uploaded");
  if (n == 0) return RTX_OK;
  if (!d_rays) return fail(c, RTX_EINVAL, "null rays");
  if (!d_ids && !d_geom) return fail(c, RTX_EINVAL, "both output buffers are null");
  KParams p;
  const rtx_status s = prep_query(c, p, n);
  if (s) return s;
  p.rays = d_rays;
  HIPCHK(c, launch_intersect(p, sph_mode(c), d_ids, d_geom, (hipStream_t)stream));
  return RTX_OK;
}

rtx_status rtx_intersect(rtx_context* c, int32_t n, const double* rays, int32_t* ids, double* geom) {
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative ray count");
  if (!c->have_scene) return fail(c, RTX_EINVAL, "no scene uploaded");
  if (n == 0) return RTX_OK;
  if (!rays) return fail(c, RTX_EINVAL, "null rays");
  if (!ids && !geom) return fail(c, RTX_EINVAL, "both output buffers are null");
  HIPCHK(c, hipSetDevice(c->device));
  const size_t rb = (size_t)n * 6 * sizeof(double);
  const size_t geom_bytes = geom ? (size_t)n * 13 * sizeof(double) : 0;
  const size_t ids_bytes = ids ? (size_t)n * 3 * sizeof(int32_t) : 0;
  rtx_status s = ensure_scratch(c, rb + geom_bytes + ids_bytes);
  if (s) return s;
  char* base = reinterpret_cast<char*>(c->d_scratch);
  double* d_rays = c->d_scratch;
  double* d_geom = geom ? reinterpret_cast<double*>(base + rb) : nullptr;
  int32_t* d_ids = ids ? reinterpret_cast<int32_t*>(base + rb + geom_bytes) : nullptr;
  HIPCHK(c, hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice));
  if ((s = rtx_intersect_device(c, n, d_rays, d_ids, d_geom, nullptr))) return s;
  // (stream-ordered blocking copies, as rtx_first_hit: no rtx_sync)
  if (geom) HIPCHK(c, hipMemcpy(geom, d_geom, geom_bytes, hipMemcpyDeviceToHost));
  if (ids) HIPCHK(c, hipMemcpy(ids, d_ids, ids_bytes, hipMemcpyDeviceToHost));
  return RTX_OK;
}

// The argument checks the device and the host form of rtx_lit_area share.  *go: there is work.
static rtx_status lit_area_args(rtx_context* c, int32_t n, const double* targets, const double* lights,
                                const double* area, const double* color, bool* go) {
  *go = false;
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative target count");
  if (!c->have_scene) return fail(c, RTX_EINVAL, "no scene uploaded");
  if (n == 0) return RTX_OK;
  if (!targets) return fail(c, RTX_EINVAL, "null targets");
  if (!area) return fail(c, RTX_EINVAL, "null area buffer");
  if (lights && color) return fail(c, RTX_EINVAL, "explicit lights have no colour: color must be null");
  if ((int64_t)n * std::max(1, c->scene.n_light) > INT32_MAX)
    return fail(c, RTX_EINVAL, "%d targets x %d lights exceed 2^31 entries", n, c->scene.n_light);
  *go = true;
  return RTX_OK;
}

rtx_status rtx_lit_area_device(rtx_context* c, int32_t n, const double* d_targets, const double* d_lights,
                               double* d_area, double* d_color, int32_t* d_status, void* stream) {
  bool go;
  rtx_status s = lit_area_args(c, n, d_targets, d_lights, d_area, d_color, &go);
  if (s || !go) return s;
  KParams p;
  if ((s = prep_query(c, p, n))) return s;
  HIPCHK(c, launch_lit_area(p, sph_mode(c), d_targets, d_lights, d_area, d_color, d_status, (hipStream_t)stream));
  return RTX_OK;
}

rtx_status rtx_lit_area(rtx_context* c, int32_t n, const double* targets, const double* lights, double* area,
                        double* color, int32_t* status) {
  bool go;
  rtx_status s = lit_area_args(c, n, targets, lights, area, color, &go);
  if (s || !go) return s;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t L = lights ? 1 : (size_t)c->scene.n_light;
  const size_t tb = (size_t)n * 3 * sizeof(double), lb = lights ? (size_t)n * 4 * sizeof(double) : 0;
  const size_t ab = (size_t)n * L * sizeof(double), cb = color ? 3 * ab : 0, sb = (size_t)n * sizeof(int32_t);
  if ((s = ensure_scratch(c, tb + lb + ab + cb + sb))) return s;
  char* base = reinterpret_cast<char*>(c->d_scratch);
  double* d_targets = c->d_scratch;
  double* d_lights = lights ? reinterpret_cast<double*>(base + tb) : nullptr;
  double* d_area = reinterpret_cast<double*>(base + tb + lb);
  double* d_color = color ? reinterpret_cast<double*>(base + tb + lb + ab) : nullptr;
  int32_t* d_status = reinterpret_cast<int32_t*>(base + tb + lb + ab + cb);   // (always: the return value needs it)
  HIPCHK(c, hipMemcpy(d_targets, targets, tb, hipMemcpyHostToDevice));
  if (lights) HIPCHK(c, hipMemcpy(d_lights, lights, lb, hipMemcpyHostToDevice));
  if ((s = rtx_lit_area_device(c, n, d_targets, d_lights, d_area, d_color, d_status, nullptr))) return s;
  // (stream-ordered blocking copies, as rtx_first_hit: no rtx_sync)
  std::vector<int32_t> st((size_t)n);
  HIPCHK(c, hipMemcpy(area, d_area, ab, hipMemcpyDeviceToHost));
  if (color) HIPCHK(c, hipMemcpy(color, d_color, cb, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(st.data(), d_status, sb, hipMemcpyDeviceToHost));
  if (status) memcpy(status, st.data(), sb);
  for (int32_t i = 0; i < n; i++)
    if (st[i]) return fail(c, (rtx_status)st[i], "%s at query %d", rtx_status_string((rtx_status)st[i]), i);
  return RTX_OK;
}

// Batched Camera#lens_func and RayTracer#rt_map (rtx_rtmap.hip).  Scene and
// camera; like the World queries they record nothing in the device's raise
// record and take no work counter or ray stack, so prep() is not theirs.
static rtx_status prep_rt_map(rtx_context* c, KParams& p, uint64_t seed) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  memset(&p, 0, sizeof p);
  p.scene = c->scene;
  p.cam = c->d_cam;
  p.seed = seed;
  p.exact_raises = (int32_t)c->opt_exact_raises;
  return RTX_OK;
}

// The argument checks of rtx_first_hit, shared by the device and the host form of rtx_lens_rays.
static rtx_status lens_rays_args(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t sample,
                                 const double* rays) {
  if (!c) return RTX_EINVAL;
  if (!rays) return fail(c, RTX_EINVAL, "null ray buffer");
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  if (x0 < 0 || y0 < 0 || x1 > c->cam.width || y1 > c->cam.height || x0 >= x1 || y0 >= y1)
    return fail(c, RTX_EINVAL, "region [%d,%d)x[%d,%d) empty or outside the %dx%d image", x0, x1, y0, y1,
                c->cam.width, c->cam.height);
  const int ms = std::max(c->cam.pre, c->cam.max_samples);
  if (sample < 0 || sample >= ms) return fail(c, RTX_EINVAL, "sample %d outside [0, %d)", sample, ms);
  return RTX_OK;
}

rtx_status rtx_lens_rays_device(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint64_t seed,
                                int32_t sample, double* d_rays, void* stream) {
  rtx_status s = lens_rays_args(c, x0, y0, x1, y1, sample, d_rays);
  if (s) return s;
  KParams p;
  if ((s = prep_rt_map(c, p, seed))) return s;
  p.x0 = x0;
  p.nx = x1 - x0;
  p.y0 = y0;
  p.nrows = y1 - y0;
  HIPCHK(c, launch_lens_rays(p, sample, d_rays, (hipStream_t)stream));
  return RTX_OK;
}

rtx_status rtx_lens_rays(rtx_context* c, int32_t x0, int32_t y0, int32_t x1, int32_t y1, uint64_t seed,
                         int32_t sample, double* rays) {
  rtx_status s = lens_rays_args(c, x0, y0, x1, y1, sample, rays);
  if (s) return s;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t bytes = (size_t)(x1 - x0) * (size_t)(y1 - y0) * 6 * sizeof(double);
  if ((s = ensure_scratch(c, bytes))) return s;
  if ((s = rtx_lens_rays_device(c, x0, y0, x1, y1, seed, sample, c->d_scratch, nullptr))) return s;
  // (a stream-ordered blocking copy, as rtx_first_hit: no rtx_sync)
  HIPCHK(c, hipMemcpy(rays, c->d_scratch, bytes, hipMemcpyDeviceToHost));
  return RTX_OK;
}

// The argument checks the device and the host form of rtx_rt_map share.  *go: there is work.
static rtx_status rt_map_args(rtx_context* c, int32_t n, const double* rays, const int32_t* keys, const int32_t* info,
                              bool* go) {
  *go = false;
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative item count");
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  if (n == 0) return RTX_OK;
  if (!rays) return fail(c, RTX_EINVAL, "null rays");
  if (!keys) return fail(c, RTX_EINVAL, "null keys");
  if (!info) return fail(c, RTX_EINVAL, "null info buffer");
  *go = true;
  return RTX_OK;
}

rtx_status rtx_rt_map_device(rtx_context* c, int32_t n, uint64_t seed, const double* d_rays, const double* d_att,
                             const int32_t* d_keys, const uint64_t* d_paths, int32_t* d_info, double* d_children,
                             uint64_t* d_child_paths, double* d_leaves, void* stream) {
  bool go;
  rtx_status s = rt_map_args(c, n, d_rays, d_keys, d_info, &go);
  if (s || !go) return s;
  KParams p;
  if ((s = prep_rt_map(c, p, seed))) return s;
  p.nrays = n;
  HIPCHK(c, launch_rt_map(p, sph_mode(c), d_rays, d_att, d_keys, d_paths, d_info, d_children, d_child_paths, d_leaves,
                          (hipStream_t)stream));
  return RTX_OK;
}

rtx_status rtx_rt_map(rtx_context* c, int32_t n, uint64_t seed, const double* rays, const double* att,
                      const int32_t* keys, const uint64_t* paths, int32_t* info, double* children,
                      uint64_t* child_paths, double* leaves) {
  bool go;
  rtx_status s = rt_map_args(c, n, rays, keys, info, &go);
  if (s || !go) return s;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t N = (size_t)n, cmax = 2 + (size_t)c->cam.pt, lmax = (size_t)std::max(1, c->scene.n_light);
  // (the 8-byte values first, then the int32 ones: every buffer 8-byte aligned)
  const size_t rb = N * 6 * sizeof(double), ab = att ? N * 3 * sizeof(double) : 0, pb = paths ? N * sizeof(uint64_t) : 0;
  const size_t cb = children ? N * cmax * 9 * sizeof(double) : 0, qb = child_paths ? N * cmax * sizeof(uint64_t) : 0;
  const size_t lb = leaves ? N * lmax * 3 * sizeof(double) : 0;
  const size_t kb = N * 4 * sizeof(int32_t), ib = N * 6 * sizeof(int32_t);
  if ((s = ensure_scratch(c, rb + ab + pb + cb + qb + lb + kb + ib))) return s;
  char* at = reinterpret_cast<char*>(c->d_scratch);
  auto take = [&](size_t bytes) {
    char* q = bytes ? at : nullptr;
    at += bytes;
    return q;
  };
  double* d_rays = reinterpret_cast<double*>(take(rb));
  double* d_att = reinterpret_cast<double*>(take(ab));
  uint64_t* d_paths = reinterpret_cast<uint64_t*>(take(pb));
  double* d_children = reinterpret_cast<double*>(take(cb));
  uint64_t* d_child_paths = reinterpret_cast<uint64_t*>(take(qb));
  double* d_leaves = reinterpret_cast<double*>(take(lb));
  int32_t* d_keys = reinterpret_cast<int32_t*>(take(kb));
  int32_t* d_info = reinterpret_cast<int32_t*>(take(ib));
  HIPCHK(c, hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice));
  if (att) HIPCHK(c, hipMemcpy(d_att, att, ab, hipMemcpyHostToDevice));
  if (paths) HIPCHK(c, hipMemcpy(d_paths, paths, pb, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_keys, keys, kb, hipMemcpyHostToDevice));
  if ((s = rtx_rt_map_device(c, n, seed, d_rays, d_att, d_keys, d_paths, d_info, d_children, d_child_paths, d_leaves,
                             nullptr)))
    return s;
  // (stream-ordered blocking copies, as rtx_first_hit: no rtx_sync)
  HIPCHK(c, hipMemcpy(info, d_info, ib, hipMemcpyDeviceToHost));
  if (children) HIPCHK(c, hipMemcpy(children, d_children, cb, hipMemcpyDeviceToHost));
  if (child_paths) HIPCHK(c, hipMemcpy(child_paths, d_child_paths, qb, hipMemcpyDeviceToHost));
  if (leaves) HIPCHK(c, hipMemcpy(leaves, d_leaves, lb, hipMemcpyDeviceToHost));
  for (int32_t i = 0; i < n; i++)
    if (info[6 * (size_t)i])
      return fail(c, (rtx_status)info[6 * (size_t)i], "%s at item %d",
                  rtx_status_string((rtx_status)info[6 * (size_t)i]), i);
  return RTX_OK;
}

rtx_status rtx_lpt_plan(const int64_t* costs, int32_t n_tiles, int32_t nranks, int32_t* plan, int32_t cap,
                        int32_t* per_rank) {
  if (n_tiles < 0 || nranks < 1 || (n_tiles > 0 && !costs) || !per_rank) return RTX_EINVAL;
  std::vector<int32_t> order(n_tiles);
  for (int32_t t = 0; t < n_tiles; t++) order[t] = t;
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return costs[a] > costs[b]; });
  std::vector<int64_t> load(nranks, 0);
  std::vector<std::vector<int32_t>> lists(nranks);
  for (int32_t t : order) {                     // to the least-loaded rank (ties: fewer tiles, lower rank)
    int r = 0;
    for (int k = 1; k < nranks; k++)
      if (load[k] < load[r] || (load[k] == load[r] && lists[k].size() < lists[r].size())) r = k;
    lists[r].push_back(t);
    load[r] += costs[t];
  }
  size_t width = 0;
  for (auto& l : lists) {
    std::sort(l.begin(), l.end());
    width = std::max(width, l.size());
  }
  *per_rank = (int32_t)width;
  if (!plan) return RTX_OK;                     // (a query of the width)
  if (cap < 0 || (size_t)cap < width) return RTX_EINVAL;   // (a negative cap: refused, not a huge size_t)
  for (int k = 0; k < nranks; k++)
    for (size_t j = 0; j < width; j++) plan[(size_t)k * width + j] = j < lists[k].size() ? lists[k][j] : n_tiles;
  return RTX_OK;
}

rtx_status rtx_render_at(rtx_context* c, int32_t x, int32_t y, uint64_t seed, double rgb[3]) {
  return rtx_render(c, x, y, x + 1, y + 1, seed, rgb, 3);
}

// ------------------------------------------------------------------ explicit rays
// rtx_trace_device with "trace_engine" -1 runs the bounce levels from this many
// rays and the lanes engine below (the smallest measured batch
// of C2 lens rays, 2^6 .. 2^20 in powers of four, at which the levels' median
// was at or below the lanes': the smallest one measured, 0.130 against 0.162 ms).
#ifndef RTX_TRACE_LEVELS_MIN_RAYS
#define RTX_TRACE_LEVELS_MIN_RAYS 64
#endif

// One trace call on `stream`: the batch buffers (level_params, as a render's,
// with "camera samples" read as "rays"; one part), then launch_trace_levels.
// The staged records are always 96 B, whatever "lv_ray_bytes" says.
// live / first: launch_trace_levels' (a ray count in device memory; the call's first trace resets the level
// statistics).  ev0: the kernel-event pairs the call's earlier traces recorded.
static rtx_status trace_levels(rtx_context* c, KParams& p, int maxs, bool levels, int32_t* d_status,
                               hipStream_t stream, const int32_t* d_live = nullptr, bool first = true, int ev0 = 0) {
  const size_t n0 = trace_items(p.nrays, batch_opts(c));
  char* buf = nullptr;
  if (rtx_status s = level_params(c, p, context_layout(c, true, levels, n0, 1, 0), 1, stream, buf)) return s;
  // the levels' overflow re-trace keeps the render's grid cap; the lanes engine takes every resident workgroup
  p.lv_redo_blocks = levels ? (int32_t)c->opt_lv_redo_blocks : 0;
  KernelEvents kev;
  if (rtx_status s = kernel_events(c, c->opt_kernel_events != 0, kev)) {
    hipFreeAsync(buf, stream);
    return s;
  }
  kev.n = ev0;
  KernelEvents* const ke = c->opt_kernel_events ? &kev : nullptr;
  const hipError_t e = launch_trace_levels(p, levels ? levels_sph_mode(c, 0) : sph_mode(c), maxs,
                                           std::max(1, c->cam.depth), (int)n0, levels, d_status, stream, ke,
                                           &c->last_plan, d_live, first);
  return launched(c, e, ke, buf, stream);
}

// RayTracer#trace_sync for n explicit rays in device buffers through the engine "trace_engine" chooses
// for a batch of n (rtx_trace_device; each pass of rtx_render_pixels_device).  p: prep()'s, with the
// ray stacks (ensure_stack).  *ran_levels: the engine that ran.
static rtx_status trace_pass(rtx_context* c, KParams p, int maxs, int32_t n, const double* d_rays,
                             const int32_t* d_keys, double* d_rgb, int32_t* d_status, hipStream_t stream,
                             bool* ran_levels, const int32_t* d_live = nullptr, bool first = true, int ev0 = 0) {
  const bool want = c->opt_trace_engine == 1 || (c->opt_trace_engine == -1 && (int64_t)n >= RTX_TRACE_LEVELS_MIN_RAYS);
  bool levels = want && levels_fit(c);
  if (levels && c->opt_lv_split != 0 && c->scene.n_light <= LV_SPLIT_MAX_LIGHTS) {
    if (c->opt_trace_engine == 1)
      return fail(c, RTX_EINVAL, "lv_split 1: explicit rays run the fused level launches only");
    levels = false;
  }
  p.rays = d_rays;
  p.keys = d_keys;
  p.nrays = n;
  p.out = d_rgb;
  *ran_levels = levels;
  return trace_levels(c, p, maxs, levels, d_status, stream, d_live, first, ev0);
}

rtx_status rtx_trace_device(rtx_context* c, int32_t n, uint64_t seed, const double* d_rays, const int32_t* d_keys,
                            double* d_rgb, int32_t* d_status, void* stream) {
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative ray count");
  if (n == 0) return RTX_OK;
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  if (!d_rays) return fail(c, RTX_EINVAL, "null rays");
  if (!d_keys) return fail(c, RTX_EINVAL, "null keys");
  if (!d_rgb) return fail(c, RTX_EINVAL, "null rgb buffer");
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  bool levels = false;
  if ((s = trace_pass(c, p, maxs, n, d_rays, d_keys, d_rgb, d_status, (hipStream_t)stream, &levels))) return s;
  c->last_trace_engine = levels ? 1 : 0;
  if (!levels) {                               // (rtx_level_stats, lv_plan_last: no level render)
    c->last_sort_levels = 0;
    c->last_plan = -1;
  }
  return RTX_OK;
}

// rtx_trace under "trace_engine" 1: upload, rtx_trace_device with a status
// buffer, download; the first raising ray by index is the call's status.
static rtx_status trace_host_levels(rtx_context* c, int32_t n, const double* rays, const int32_t* keys, uint64_t seed,
                                    double* out) {
  HIPCHK(c, hipSetDevice(c->device));
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  // as the lanes path: wait for the context's earlier work (it may still read the scratch buffer
  // that is reused and perhaps reallocated below) and discard the raises nobody collected
  rtx_sync(c, nullptr);
  const size_t rb = sizeof(double) * 6 * n, kb = sizeof(int32_t) * 3 * n, ob = sizeof(double) * 3 * n,
               sb = sizeof(int32_t) * (size_t)n;
  rtx_status s = ensure_scratch(c, rb + ob + kb + sb + 64);
  if (s) return s;
  char* base = (char*)c->d_scratch;
  double* d_rays = (double*)base;
  double* d_out = (double*)(base + rb);
  int32_t* d_keys = (int32_t*)(base + rb + ob);
  int32_t* d_status = (int32_t*)(base + rb + ob + kb);
  HIPCHK(c, hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_keys, keys, kb, hipMemcpyHostToDevice));
  if ((s = rtx_trace_device(c, n, seed, d_rays, d_keys, d_out, d_status, nullptr))) return s;
  std::vector<int32_t> st((size_t)n);
  HIPCHK(c, hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(st.data(), d_status, sb, hipMemcpyDeviceToHost));
  int32_t first = -1, kinds = 0;
  for (int32_t i = 0; i < n; i++)
    if (st[i]) {
      if (first < 0) first = i;
      kinds |= 1 << st[i];
    }
  if (first < 0) return RTX_OK;
  const rtx_status r = (rtx_status)st[first];
  return fail(c, r, "%s at ray %llu%s", rtx_status_string(r), (unsigned long long)first,
              __builtin_popcount(kinds) > 1 ? " (and other errors)" : "");
}

// ------------------------------------------------------------------ pixel lists
// Camera#render_at for the n pixels d_xy: the list in chunks of
// P pixels with P * max(pre, max - pre) <= "lv_batch", so that each pass of a
// chunk is one batch of the engine; per chunk the lens rays of the pre samples
// (k_pixel_rays), their trace, render_at's pixel stage (k_pixel_reduce), and
// with max > pre the extra samples of the pixels it listed: their rays
// (k_pixel_extra_rays), a trace launched for the chunk's capacity whose live
// ray count stays in device memory, and k_pixel_finish.  All on `stream`,
// nothing read back.  The chunk buffers (rtx_launch.h PixelBufs) are one
// stream-ordered allocation reused by every chunk, beside the engine's own.
rtx_status rtx_render_pixels_device(rtx_context* c, int32_t n, uint64_t seed, const int32_t* d_xy, double* d_rgb,
                                    double* d_variance, int32_t* d_info, void* hip_stream) {
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative pixel count");
  if (n == 0) return RTX_OK;
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  if (!d_xy) return fail(c, RTX_EINVAL, "null pixel list");
  if (!d_rgb) return fail(c, RTX_EINVAL, "null rgb buffer");
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  const hipStream_t stream = (hipStream_t)hip_stream;
  const int pre = p.pre, mx = p.max_samples, n_extra = std::max(0, mx - pre);
  const int64_t per = std::max(pre, n_extra);
  const int32_t P = (int32_t)std::max<int64_t>(1, std::min<int64_t>(n, c->opt_lv_batch / per));
  const size_t cap = (size_t)P * (size_t)per;
  const size_t rb = al256(cap * 6 * sizeof(double)), cb = al256(cap * 3 * sizeof(double)),
               kb = al256(cap * 3 * sizeof(int32_t)), sb = al256(cap * sizeof(int32_t)),
               lb = al256((size_t)P * sizeof(int32_t));
  char* buf = nullptr;
  HIPCHK(c, hipMallocAsync((void**)&buf, rb + cb + kb + sb + lb + 256, stream));
  const PixelBufs b{(double*)buf, (int32_t*)(buf + rb + cb), (double*)(buf + rb), (int32_t*)(buf + rb + cb + kb),
                    (int32_t*)(buf + rb + cb + kb + sb), (int32_t*)(buf + rb + cb + kb + sb + lb)};
  hipError_t e = hipSuccess;
  bool first = true, any_levels = false;
  for (int32_t i0 = 0; i0 < n && e == hipSuccess && !s; i0 += P) {
    const int32_t m = std::min(P, n - i0);
    const int32_t* xy = d_xy + 2 * (size_t)i0;
    double* rgb = d_rgb + 3 * (size_t)i0;
    double* var = d_variance ? d_variance + i0 : nullptr;
    int32_t* info = d_info ? d_info + 2 * (size_t)i0 : nullptr;
    bool levels = false;
    e = launch_pixel_rays(c->d_cam, seed, xy, m, pre, b, stream);
    if (e != hipSuccess) break;
    p.work = c->d_work + (c->work_seq++ % RTX_WORK_RING);
    if ((s = trace_pass(c, p, maxs, m * pre, b.rays, b.keys, b.col, b.st, stream, &levels, nullptr, first,
                        first ? 0 : c->n_ev)))
      break;
    if (first) c->last_trace_engine = levels ? 1 : 0;   // ("trace_engine_last": the engine of the call's first pass)
    any_levels = any_levels || levels;
    first = false;
    e = launch_pixel_reduce(c->d_cam, m, pre, mx, b, rgb, var, info, stream);
    if (e != hipSuccess || n_extra == 0) continue;
    e = launch_pixel_extra_rays(c->d_cam, seed, xy, m, pre, mx, b, stream);
    if (e != hipSuccess) break;
    p.work = c->d_work + (c->work_seq++ % RTX_WORK_RING);
    if ((s = trace_pass(c, p, maxs, m * n_extra, b.rays, b.keys, b.col, b.st, stream, &levels, b.count + 1, false,
                        c->n_ev)))
      break;
    any_levels = any_levels || levels;
    e = launch_pixel_finish(m, pre, mx, b, rgb, info, stream);
  }
  if (!any_levels) {                           // (rtx_level_stats, lv_plan_last: no level render)
    c->last_sort_levels = 0;
    c->last_plan = -1;
  }
  const hipError_t f = hipFreeAsync(buf, stream);
  if (s) return s;
  HIPCHK(c, e);
  HIPCHK(c, f);
  return RTX_OK;
}

// The host form: upload, rtx_render_pixels_device, download; the first raising
// pixel by index is the call's status.
rtx_status rtx_render_pixels(rtx_context* c, int32_t n, uint64_t seed, const int32_t* xy, double* rgb,
                             double* variance, int32_t* info) {
  if (!c) return RTX_EINVAL;
  if (n < 0) return fail(c, RTX_EINVAL, "negative pixel count");
  if (n == 0) return RTX_OK;
  if (!c->have_scene || !c->have_cam) return fail(c, RTX_EINVAL, "no scene or camera uploaded");
  if (!xy) return fail(c, RTX_EINVAL, "null pixel list");
  if (!rgb) return fail(c, RTX_EINVAL, "null rgb buffer");
  HIPCHK(c, hipSetDevice(c->device));
  // as trace_host_levels: wait for the context's earlier work (it may still read the scratch buffer
  // that is reused and perhaps reallocated below) and discard the raises nobody collected
  rtx_sync(c, nullptr);
  const size_t N = (size_t)n, ob = N * 3 * sizeof(double), vb = N * sizeof(double), xb = N * 2 * sizeof(int32_t);
  rtx_status s = ensure_scratch(c, ob + vb + 2 * xb + 64);
  if (s) return s;
  char* base = (char*)c->d_scratch;
  double* d_rgb = (double*)base;
  double* d_var = (double*)(base + ob);
  int32_t* d_xy = (int32_t*)(base + ob + vb);
  int32_t* d_info = (int32_t*)(base + ob + vb + xb);
  HIPCHK(c, hipMemcpy(d_xy, xy, xb, hipMemcpyHostToDevice));
  if ((s = rtx_render_pixels_device(c, n, seed, d_xy, d_rgb, variance ? d_var : nullptr, d_info, nullptr))) return s;
  std::vector<int32_t> st;
  int32_t* inf = info;
  if (!inf) {
    st.resize(2 * N);
    inf = st.data();
  }
  HIPCHK(c, hipMemcpy(rgb, d_rgb, ob, hipMemcpyDeviceToHost));
  if (variance) HIPCHK(c, hipMemcpy(variance, d_var, vb, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(inf, d_info, xb, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < N; i++)
    if (inf[2 * i]) {
      const rtx_status r = (rtx_status)inf[2 * i];
      return fail(c, r, "%s at pixel %zu (%d, %d)", rtx_status_string(r), i, xy[2 * i], xy[2 * i + 1]);
    }
  return RTX_OK;
}

rtx_status rtx_trace(rtx_context* c, int32_t n, const double* rays, const int32_t* keys, uint64_t seed,
                     double* out) {
  if (!c || n < 0 || (n && (!rays || !keys || !out))) return fail(c, RTX_EINVAL, "bad arguments");
  if (n == 0) return RTX_OK;
  if (c->opt_trace_engine == 1) return trace_host_levels(c, n, rays, keys, seed, out);
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  c->last_trace_engine = 0;
  rtx_sync(c, nullptr);
  hipSetDevice(c->device);
  const size_t rb = sizeof(double) * 6 * n, kb = sizeof(int32_t) * 3 * n, ob = sizeof(double) * 3 * n;
  if ((s = ensure_scratch(c, rb + kb + ob + 64))) return s;
  char* base = (char*)c->d_scratch;
  double* d_rays = (double*)base;
  double* d_out = (double*)(base + rb);
  int32_t* d_keys = (int32_t*)(base + rb + ob);
  HIPCHK(c, hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpy(d_keys, keys, kb, hipMemcpyHostToDevice));
  p.out = d_out;
  p.rays = d_rays;
  p.keys = d_keys;
  p.nrays = n;
  HIPCHK(c, launch_trace(p, sph_mode(c), maxs, nullptr));
  HIPCHK(c, hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost));
  c->err_keys_rays = true;
  const rtx_status st = rtx_sync(c, nullptr);
  c->err_keys_rays = false;
  return st;
}

rtx_status rtx_path_trace(rtx_context* c, int32_t n, const double* rays, double* out) {
  if (!c || n < 0 || (n && (!rays || !out))) return fail(c, RTX_EINVAL, "bad arguments");
  if (n == 0) return RTX_OK;
  KParams p;
  rtx_status s = prep(c, p, 1);
  if (s) return s;
  rtx_sync(c, nullptr);
  hipSetDevice(c->device);
  const size_t rb = sizeof(double) * 6 * n, ob = sizeof(double) * 3 * n;
  if ((s = ensure_scratch(c, rb + ob))) return s;
  double* d_rays = c->d_scratch;
  double* d_out = c->d_scratch + 6 * (size_t)n;
  HIPCHK(c, hipMemcpy(d_rays, rays, rb, hipMemcpyHostToDevice));
  p.out = d_out;
  p.rays = d_rays;
  p.nrays = n;
  HIPCHK(c, launch_path_trace(p, nullptr));
  HIPCHK(c, hipMemcpy(out, d_out, ob, hipMemcpyDeviceToHost));
  c->err_keys_rays = true;
  const rtx_status st = rtx_sync(c, nullptr);
  c->err_keys_rays = false;
  return st;
}

rtx_status rtx_count_work(rtx_context* c, uint64_t seed, uint64_t counts[RTX_NCOUNT]) {
  if (!c || !counts) return fail(c, RTX_EINVAL, "null argument");
  KParams p;
  rtx_status s = prep(c, p, seed);
  if (s) return s;
  int maxs = 0;
  if ((s = required_stack(c, maxs))) return s;
  if ((s = ensure_stack(c, p, maxs))) return s;
  hipSetDevice(c->device);
  const int W = c->cam.width, H = c->cam.height;
  if ((s = ensure_scratch(c, sizeof(double) * 3 * (size_t)W * H))) return s;
  HIPCHK(c, hipMemset(c->d_counts, 0, sizeof(unsigned long long) * RTX_NCOUNT));
  p.x0 = 0;
  p.nx = W;
  p.nrows = H;
  p.out = c->d_scratch;
  p.stride = (size_t)W * 3;
  if ((s = render_region(c, p, true, maxs, nullptr))) return s;
  HIPCHK(c, hipDeviceSynchronize());
  unsigned long long tmp[RTX_NCOUNT];
  HIPCHK(c, hipMemcpy(tmp, c->d_counts, sizeof tmp, hipMemcpyDeviceToHost));
  for (int k = 0; k < RTX_NCOUNT; k++) counts[k] = tmp[k];
  return rtx_sync(c, nullptr);
}

rtx_status rtx_quantize_device(const double* d_rgb, int32_t w, int32_t h, size_t stride, int32_t blend,
                               uint8_t* d_out, void* stream) {
  if (w < 0 || h < 0 || stride < (size_t)w * 3 || (w * h && (!d_rgb || !d_out))) return RTX_EINVAL;
  return launch_quantize(d_rgb, w, h, stride, blend, d_out, (hipStream_t)stream) == hipSuccess ? RTX_OK
                                                                                                 : RTX_EHIP;
}

rtx_status rtx_quantize(const double* rgb, int32_t w, int32_t h, size_t stride, int32_t blend, uint8_t* out) {
  if (w < 0 || h < 0 || stride < (size_t)w * 3 || (w * h && (!rgb || !out))) return RTX_EINVAL;
  if (w * h == 0) return RTX_OK;
  double* d_in = nullptr;
  uint8_t* d_o = nullptr;
  const size_t ib = sizeof(double) * stride * h, ob = (size_t)w * h * 4;
  rtx_status s = RTX_OK;
  if (hipMalloc(&d_in, ib) != hipSuccess || hipMalloc(&d_o, ob) != hipSuccess ||
      hipMemcpy(d_in, rgb, ib, hipMemcpyHostToDevice) != hipSuccess ||
      launch_quantize(d_in, w, h, stride, blend, d_o, nullptr) != hipSuccess ||
      hipMemcpy(out, d_o, ob, hipMemcpyDeviceToHost) != hipSuccess)
    s = RTX_EHIP;
  hipFree(d_in);
  hipFree(d_o);
  return s;
}

// ------------------------------------------------------------------ Vec3 API
static rtx_vec3 mk(V3 a) {
  rtx_vec3 r;
  r.v[0] = a.x;
  r.v[1] = a.y;
  r.v[2] = a.z;
  r.r = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);      // Vec3_c_create (fast_4d_matrix.c:62-73)
  return r;
}
static V3 un(rtx_vec3 a) { return v3(a.v[0], a.v[1], a.v[2]); }

rtx_vec3 rtx_vec3_from_a(double x, double y, double z) { return mk(v3(x, y, z)); }
double rtx_vec3_r(rtx_vec3 a) { return a.r; }
double rtx_vec3_r2(rtx_vec3 a) { return a.r * a.r; }
double rtx_vec3_dot(rtx_vec3 a, rtx_vec3 b) { return vdot(un(a), un(b)); }
rtx_status rtx_vec3_cos(rtx_vec3 a, rtx_vec3 b, double* out) {
  uint32_t err = 0;
  double v = vcos(un(a), un(b), err);
  if (out) *out = v;
  return err ? RTX_EZERO_VEC : RTX_OK;
}
rtx_vec3 rtx_vec3_cross(rtx_vec3 a, rtx_vec3 b) { return mk(vcross(un(a), un(b))); }
rtx_vec3 rtx_vec3_add(rtx_vec3 a, rtx_vec3 b) { return mk(vadd(un(a), un(b))); }
rtx_vec3 rtx_vec3_sub(rtx_vec3 a, rtx_vec3 b) { return mk(vsub(un(a), un(b))); }
rtx_vec3 rtx_vec3_mul(rtx_vec3 a, rtx_vec3 b) { return mk(vmul(un(a), un(b))); }
rtx_vec3 rtx_vec3_scale(rtx_vec3 a, double s) { return mk(vsc(un(a), s)); }
rtx_vec3 rtx_vec3_div(rtx_vec3 a, double s) { return mk(vdiv(un(a), s)); }
rtx_vec3 rtx_vec3_neg(rtx_vec3 a) { return mk(vneg(un(a))); }
rtx_vec3 rtx_vec3_pos(rtx_vec3 a) { return mk(un(a)); }
rtx_status rtx_vec3_normalize(rtx_vec3 a, rtx_vec3* out) {
  uint32_t err = 0;
  V3 v = vnorm(un(a), err);
  if (err) return RTX_EZERO_VEC;
  if (out) *out = mk(v);
  return RTX_OK;
}
// The bang forms mutate in place and recompute r (Vec3_c_recalc_r, :226-229);
// as values they equal the non-bang results.
rtx_vec3 rtx_vec3_add_bang(rtx_vec3 a, rtx_vec3 b) { return mk(vadd(un(a), un(b))); }
rtx_vec3 rtx_vec3_sub_bang(rtx_vec3 a, rtx_vec3 b) { return mk(vsub(un(a), un(b))); }
rtx_vec3 rtx_vec3_mul_bang(rtx_vec3 a, rtx_vec3 b) { return mk(vmul(un(a), un(b))); }
rtx_vec3 rtx_vec3_mul_bang_scalar(rtx_vec3 a, double s) { return mk(vsc(un(a), s)); }

double rtx_rand(uint64_t seed, int32_t x, int32_t y, int32_t sample, uint64_t path, int32_t draw) {
  return rand01(seed, x, y, sample, path, draw);
}

}  // extern "C"
