// rtx_batch.h — the batch of the bounce-level engine:
// its level-0 items, the capacities of its queues and record arena, and where
// every buffer of a part's set sits in the one allocation a call makes.
// Host-only arithmetic over a few scalars and option values, plain C++ (g++
// -std=c++17, as rtx_plan.h and rtx_sched.h): both entries of the engine
// (rtx_capi.cpp render_levels and trace_levels) and tools/scene_dump.cpp
// --buffers call this one copy (tests/test_level_buffers.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "rtx_plan.h"
#include "rtx_sched.h"                          // LV_ROUND_MAX, lv_static_chunks, lv_round_chunk (host and device)

namespace rtx {

// One launch per tree level (or three, option lv_split).  The ray queue of
// every level >= 1 (and the hit queue of the split phases) is cut into
// LV_SLICES slices of 2^k slots, each with its own allocation counter on its
// own 128-B line (no contended device atomics).
constexpr int LV_MAXL = 64;                     // levels (= trace_depth) the engine supports
constexpr int LV_SLICES = 64;                   // slices per queue (one per lane of a consumer wave)
constexpr int LV_CLAIMS = 16;                   // sharded chunk-claim counters per launch
constexpr int LV_DONE = 16;                     // wave-completion counters per level launch (lv_level_done)
constexpr int LV_CELL_BITS_MAX = 4;             // ray bins (option lv_sort): origin cells per axis = 2^lv_cell_bits
constexpr int LV_BINS = 8 << (3 * LV_CELL_BITS_MAX); // x 8 direction octants: at most 32,768 bins
constexpr int LV_MAX_PARTS = 4;                 // parts of a region rendered at once (option lv_streams), at most
constexpr size_t RAY_BYTES = 96;                // staged ray record of the bounce-level engine (at most)
constexpr size_t LV_HIT_BYTES = 64;             // split phases: hit-queue record

struct LevelCtl {
  uint32_t count0;                              // level-0 items of the batch
  uint32_t redo_n;                              // level-0 items handed to the lanes engine (capacity overflow)
  uint32_t dropped;                             // child rays that found no room (diagnostic)
  uint32_t hl_n;                                // highlight rays whose lit_area raise check is deferred (k_hl_raise)
  uint32_t pad[27];                             // (pad[0]: the lanes-engine work counter of parts 1..)
  uint32_t sc[LV_MAXL + 1][LV_SLICES * 32];     // rays allocated in slice s of level d: sc[d][32 s]
  uint32_t sh[LV_MAXL + 1][LV_SLICES * 32];     // split phases: hits of level d in slice s
  uint32_t claim[3][LV_MAXL + 1][LV_CLAIMS * 32]; // chunk claims: [launch kind: fused/trace, shadow, shade][level][j * 32]
  // compact layout of level d (written by the last workgroup of the launch that allocated it)
  uint32_t lay_cnt[LV_MAXL + 2][LV_SLICES];     // rays in slice s (clamped to the slice)
  uint32_t lay_pex[LV_MAXL + 2][LV_SLICES];     // exclusive ray prefix of slice s
  uint32_t lay_cin[LV_MAXL + 2][LV_SLICES];     // inclusive 64-ray chunk prefix of slice s
  uint32_t lay_base[LV_MAXL + 2];               // first record of level d in the arena
  uint32_t done[LV_MAXL + 2];                   // completed done_sub counters of the launch allocating level d
  uint32_t done_sub[LV_MAXL + 1][LV_DONE * 32]; // finished waves w (w mod LV_DONE = j) of that launch: [d][32 j]
};

// Tree-record bytes for a scene with n_light lights (one leaf per fired light).
inline int levels_rec_bytes(int n_light) {
  const int nl = n_light > 1 ? n_light : 1;
  return (8 + 24 * nl + 15) & ~15;       // {meta, first child} + one leaf per fired light
}

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// The options the layout reads, with the context's defaults (rtx_capi.cpp takes its own from here).
struct BatchOpts {
  int64_t lv_batch = 1 << 24;      // level-0 items (camera samples) per batch (C4: 2^23 -> 2^24 358.0 -> 352.8 ms,
                                   // half the level launches and their tails, r08k)
  int64_t lv_stage_pct = 300;      // ray records per staging buffer, % of the batch items
  int64_t lv_rec_pct = 1600;       // tree records of a batch (all levels), % of the batch items
  int64_t lv_floor = 1 << 20;      // at least this many staging and 4x this many tree records
  int64_t lv_streams = 2;          // P = the region's tiles in P interleaved parts on P streams at once
  int64_t lv_split = PlanOpts{}.lv_split;   // 1 = three phase launches per level (trace / shadow / shade)
  int64_t lv_hl_cap = 0;           // deferred highlight-check list entries (0 auto)
  int64_t lv_sort = -1;            // 1 = levels visited bin by bin (direction octant, origin cell), 0 off,
                                   // -1 auto = on
  int64_t lv_sort_from = 0;        // the first level binned; 0 auto: level 1 above 512 spheres (C4 354 -> 307 ms), else
                                   // the last level only (C2 4.60 -> 4.57 ms; all levels 4.65 -> 4.88, r10d/r10k)
  int64_t lv_sort_copy = 0;        // 1 = binning copies the rays' records into bin order (r11i: C4 296 -> 342 ms, off)
  int64_t lv_ray_bytes = 0;        // staged ray record, 0 auto (80 B when every path fits 32 bits), 80, 96
};

// The level-0 items of a render's batch over a region of `tiles` 8x8 tiles,
// rendered in `parts` interleaved parts at once (lv_streams): pass 0 (tiles) or
// pass 1 (>= one pixel's extra samples).  (pre >= 1: rtx_camera_set refuses
// anything else, so no caller needs a max(1, pre) of its own.)
struct BatchItems {
  int parts, batch_tiles;
  size_t n0;
};
inline BatchItems batch_items(int64_t tiles, int pre, int max_samples, const BatchOpts& o) {
  const int64_t per_tile = 64 * (int64_t)pre;
  const int64_t parts = std::max<int64_t>(1, std::min<int64_t>(o.lv_streams, tiles));
  const int64_t batch_tiles = std::max<int64_t>(1, std::min<int64_t>(o.lv_batch / per_tile, (tiles + parts - 1) / parts));
  return BatchItems{(int)parts, (int)batch_tiles,
                    std::max((size_t)(batch_tiles * per_tile), (size_t)std::max(0, max_samples - pre))};
}
// The same for a trace call of `nrays` explicit rays: one part, batches of lv_batch rays.
inline size_t trace_items(int64_t nrays, const BatchOpts& o) {
  return (size_t)std::max<int64_t>(1, std::min<int64_t>(o.lv_batch, nrays));
}

// 80-B ray records when a ray's path id fits 32 bits at every level: path
// < (pt + 3)^trace_depth (the path ids of rtx_device.h emit / lv_finish).
// lv_ray_bytes 80 asked for a camera whose paths do not fit is refused, not
// truncated.
inline bool lv_paths32(int depth, int pt) {
  uint64_t v = 1;
  for (int l = 0; l < depth; l++) {
    v *= (uint64_t)pt + 3;
    if (v > (1ull << 32)) return false;
  }
  return true;
}

inline bool lv_split_on(int n_light, const BatchOpts& o) { return o.lv_split != 0 && n_light <= LV_SPLIT_MAX_LIGHTS; }

// ray binning (option lv_sort) for the fused level launches
// The first level binned (0: none).  Large scenes bin every level >= 1 (C4
// 354 -> 307 ms); small ones only the last, where the rays are most incoherent
// and most numerous (C2: binning every level costs more than it gains, r10d;
// the last level alone gains 0.5 %, r10k).
// n0: the level-0 items of a batch (the last level of a small scene is binned
// only from 2^22 of them: a 1/8 or 1/4 share of the C2 frame lost 4-5 % to the
// binning passes' fixed cost, half of it neither gained nor lost, r10p).
inline int sort_from(int n_sphere, int n_light, int depth, size_t n0, const BatchOpts& o) {
  if (o.lv_sort == 0 || lv_split_on(n_light, o)) return 0;
  const bool large = n_sphere > 512;
  if (o.lv_sort == -1 && o.lv_sort_from == 0 && !large && n0 < ((size_t)1 << 22)) return 0;
  const int from = o.lv_sort_from > 0 ? (int)o.lv_sort_from : large ? 1 : depth - 1;
  return from >= 1 && from < depth ? from : 0;
}

// The buffers of one part's set, in the order they are carved.
enum BatchBuf {
  LB_CTL, LB_REDO_OF, LB_REDO_LIST, LB_REDO_SMP, LB_STAGE0, LB_STAGE1, LB_REC, LB_HIT, LB_AREA, LB_HLQ, LB_KEY, LB_PERM,
  LB_BINS, LB_SORTED, LB_COUNT
};
constexpr const char* BATCH_BUF_NAMES[LB_COUNT] = {"ctl", "redo_of", "redo_list", "redo_smp", "stage0", "stage1", "rec",
                                                   "hit", "area", "hlq", "key", "perm", "bins", "sorted"};

// What a call asks of the layout.  n0: the level-0 items of a batch, camera
// samples of a render (batch_items) or rays of a trace call (trace_items).
struct BatchIn {
  bool trace;                      // rtx_trace_device: one part, no split buffers, 96-B staged records, a 256-B tail
  bool levels;                     // false (trace calls only): the lanes engine runs the batch, no level buffers
  size_t n0;
  int parts;                       // sets (a trace call: 1)
  size_t npx;                      // render: pixels of the region (the extra-sample list of the tail)
  int n_sphere, n_light, depth, pt;
};

struct BatchLayout {
  const char* refusal = nullptr;   // non-null: the call is refused with this message, nothing else is set
  size_t scap = 0;                 // ray records per staging buffer (levels >= 1): LV_SLICES << slog2
  int slog2 = 0;
  size_t lcap = 0;                 // tree records of the arena
  size_t hcap = 0;                 // split phases: hits per level, LV_SLICES << hlog2
  int hlog2 = 0;
  size_t hlcap = 0;                // entries of the deferred highlight list (0: no list)
  int rec_bytes = 0;
  int sort_from = 0;               // the first level binned (0: none)
  bool sort_copy = false;
  bool split = false;
  int ray_dbl = 12;                // staged ray record, doubles (KParams::lv_ray_dbl)
  size_t off[LB_COUNT] = {};       // byte offset of each buffer within a set (each a multiple of 256)
  size_t size[LB_COUNT] = {};      // its bytes (a multiple of 256; 0: nothing to hold)
  bool present[LB_COUNT] = {};     // false: the kernels get a null pointer for it
  size_t set = 0;                  // bytes of one part's set
  size_t tail = 0;                 // after the last set: the extra-sample count (64 words) and, renders, list
  size_t total = 0;                // parts * set + tail: the call's allocation
};

inline BatchLayout batch_layout(const BatchIn& in, const BatchOpts& o) {
  BatchLayout L;
  const size_t n0 = in.n0, fl = (size_t)o.lv_floor;
  const size_t want = std::max<size_t>(std::max<size_t>(64, fl), n0 * (size_t)o.lv_stage_pct / 100);
  L.lcap = std::max<size_t>(std::max(n0, 4 * fl), n0 * (size_t)o.lv_rec_pct / 100);
  // queues of levels >= 1: LV_SLICES slices of 2^k slots (k rounded up)
  while (((size_t)LV_SLICES << L.slog2) < want) L.slog2++;
  L.scap = (size_t)LV_SLICES << L.slog2;
  if (in.levels && (L.scap > UINT32_MAX / 2 || L.lcap > UINT32_MAX / 2)) {
    L.refusal = "bounce-level buffers exceed 2^31 records: lower lv_batch";
    return L;
  }
  // (a trace call's records are always 96 B: the 80-B record decodes the RNG key from a camera item,
  // which an explicit ray is not)
  const bool path32 = lv_paths32(in.depth, in.pt);
  if (!in.trace && o.lv_ray_bytes == 80 && !path32) {
    L.refusal = "lv_ray_bytes 80: this camera's ray paths need 64 bits ((pt + 3)^trace_depth > 2^32)";
    return L;
  }
  L.ray_dbl = (in.trace || o.lv_ray_bytes == 96 || !path32) ? 12 : 10;
  L.rec_bytes = levels_rec_bytes(in.n_light);
  // deferred highlight checks (k_hl_raise): room for 1/256 of the batch's tree
  // records (rays; C2 fires on ~0.1 % of them); a ray that finds the list full
  // has its sample re-rendered by the lanes engine (option lv_hl_cap: the size)
  L.hlcap = !in.levels ? 0 : o.lv_hl_cap > 0 ? (size_t)o.lv_hl_cap : std::max<size_t>(4096, L.lcap / 256);
  // split phases: the hit queue of a level (at most its rays) and its shadow results
  L.split = !in.trace && lv_split_on(in.n_light, o);
  if (!in.trace)
    while (((size_t)LV_SLICES << L.hlog2) < std::max(n0, L.scap)) L.hlog2++;
  L.hcap = (size_t)LV_SLICES << L.hlog2;
  // ray binning (lv_sort, fused levels only): a bin per staged slot, the
  // level's bin list, the bin counts and cursors
  L.sort_from = in.levels ? sort_from(in.n_sphere, in.n_light, in.depth, n0, o) : 0;
  const bool sort = L.sort_from > 0;
  // (lv_sort_copy: the binned level's records in bin order, a third staging buffer)
  L.sort_copy = sort && o.lv_sort_copy == 1;
  const size_t sz_redo = al256(n0 * 4), sz_stage = in.levels ? al256(L.scap * RAY_BYTES) : 0;
  const struct { size_t bytes; bool present; } bufs[LB_COUNT] = {
      {al256(sizeof(LevelCtl)), true},
      {sz_redo, true},
      {sz_redo, true},
      {al256(n0 * 32), true},
      {sz_stage, true},                        // (not levels: empty, the pointers stay set)
      {sz_stage, true},
      {in.levels ? al256(L.lcap * (size_t)L.rec_bytes) : 0, true},
      {L.split ? al256(L.hcap * LV_HIT_BYTES) : 0, L.split},
      {L.split ? al256(L.hcap * (size_t)std::max(1, in.n_light) * 16) : 0, L.split},
      {al256(L.hlcap * 64), in.levels},
      {sort ? al256(L.scap * 2) : 0, sort},
      {sort ? al256(L.scap * 8) : 0, sort},
      {sort ? al256((size_t)LV_BINS * 8) : 0, sort},
      {L.sort_copy ? sz_stage : 0, L.sort_copy}};
  for (int k = 0; k < LB_COUNT; k++) {
    L.off[k] = L.set;
    L.size[k] = bufs[k].bytes;
    L.present[k] = bufs[k].present;
    L.set += bufs[k].bytes;
  }
  L.tail = in.trace ? 256 : al256((in.npx + 64) * 4);
  L.total = (size_t)in.parts * L.set + L.tail;
  return L;
}

}  // namespace rtx
