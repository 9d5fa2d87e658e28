// scene_dump.cpp — prints what rtx_scene_upload would send for a world YAML
// (tests/test_scene_build.py).  Runs build_host_scene (rtx_scene_build.h) and
// prints one line per device array, "array <name> <bytes> <64-bit FNV-1a>",
// then the scalars of SceneDev, "scalar <name> <value>" (floats as %a).
// Host code only, no GPU call.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -o scene_dump tools/scene_dump.cpp -lz -lpthread
//   scene_dump scenes/c2_world.yml [sah: 1 (default) or 0]
//
// scene_dump --plan world.yml...: instead, per world, one line "plan <packed plan>
// <name> <value> ..." with the launch plan of its fused level launches under default
// options (rtx_plan.h fused_plan, the arithmetic the launcher runs; the read-only option
// lv_plan_last reports the same integer after a render) and the scalars it depends on;
// "status <code> <message>" for a world the host build refuses (tests/test_level_plans.py).
//
// scene_dump --buffers [case...]: no world; per case (an argument, or a line of stdin when
// there is no argument) one line of "name value" pairs with the batch and the buffer layout
// of a bounce-level call (rtx_batch.h batch_items / trace_items / batch_layout, the arithmetic
// rtx_capi.cpp runs) and sizeof(LevelCtl) (tests/test_level_buffers.py).  A case is 21
// integers: trace (0 render, 1 trace), the region's 8x8 tiles (render), its pixels or the
// call's rays, pre, max_samples, trace_depth, pt, n_sphere, n_light, levels (0: a trace call
// through the lanes engine), then BatchOpts' fields in their order: lv_batch lv_stage_pct
// lv_rec_pct lv_floor lv_streams lv_split lv_hl_cap lv_sort lv_sort_from lv_sort_copy
// lv_ray_bytes.  A refusal's message is printed with '_' for its spaces ("-": none).
#include <stdio.h>
#include <string.h>

#include "../raytracing_rb_amd/cli/scene_load.hpp"
#include "../raytracing_rb_amd/csrc/rtx_batch.h"
#include "../raytracing_rb_amd/csrc/rtx_plan.h"
#include "../raytracing_rb_amd/csrc/rtx_scene_build.h"

using namespace rtx;

static uint64_t fnv1a(const void* p, size_t n) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* b = (const unsigned char*)p;
  for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

template <typename T>
static void array(const char* name, const std::vector<T>& v) {
  printf("array %s %zu %016llx\n", name, v.size() * sizeof(T), (unsigned long long)fnv1a(v.data(), v.size() * sizeof(T)));
}

static int plans(int n, char** worlds) {
  for (int k = 0; k < n; k++) {
    rtxcli::Scene sc;
    rtxcli::load_world(worlds[k], sc);
    HostScene H;
    std::string msg;
    const rtx_status st = build_host_scene(&sc.desc, true, H, msg);
    if (st != RTX_OK) {
      printf("status %d %s\n", (int)st, msg.c_str());
      continue;
    }
    const SceneDev& S = H.dev;
    printf("plan %lld", (long long)fused_plan(S, PlanOpts{}));
#define I(f) printf(" " #f " %d", (int)S.f)
    I(n_sphere), I(n_light), I(n_obj), I(n_nodes), I(n_slots), I(bvh_stack), I(q_ok);
    I(lbuf_n), I(lbuf_stride), I(rbuf_n), I(rgate_stride), I(rbuf_sphere);
#undef I
    printf("\n");
  }
  return 0;
}

// One --buffers case -> one line of "name value" pairs: the level-0 items of a batch and the layout of
// the call's buffers (rtx_batch.h), as rtx_capi.cpp asks for them.
static int buffers_case(const char* text) {
  long long v[21];
  int n = 0, used = 0;
  for (const char* q = text; n < 21 && sscanf(q, "%lld%n", &v[n], &used) == 1; q += used) n++;
  if (n != 21) {
    fprintf(stderr, "--buffers: a case is 21 integers (%d read): %s\n", n, text);
    return 2;
  }
  const bool trace = v[0] != 0, levels = v[9] != 0;
  const int pre = (int)v[3], max_samples = (int)v[4];
  BatchOpts o;
  o.lv_batch = v[10], o.lv_stage_pct = v[11], o.lv_rec_pct = v[12], o.lv_floor = v[13], o.lv_streams = v[14];
  o.lv_split = v[15], o.lv_hl_cap = v[16], o.lv_sort = v[17], o.lv_sort_from = v[18], o.lv_sort_copy = v[19];
  o.lv_ray_bytes = v[20];
  BatchItems it{1, 0, 0};
  if (trace) it.n0 = trace_items(v[2], o);
  else it = batch_items(v[1], pre, max_samples, o);
  const BatchLayout L = batch_layout(
      BatchIn{trace, levels, it.n0, it.parts, trace ? 0 : (size_t)v[2], (int)v[7], (int)v[8], (int)v[5], (int)v[6]}, o);
  std::string why = L.refusal ? L.refusal : "-";
  for (char& ch : why)
    if (ch == ' ') ch = '_';
  printf("sizeof_LevelCtl %zu parts %d batch_tiles %d n0 %zu refusal %s", sizeof(LevelCtl), it.parts, it.batch_tiles, it.n0,
         why.c_str());
  printf(" scap %zu slog2 %d lcap %zu hcap %zu hlog2 %d hlcap %zu rec_bytes %d sort_from %d sort_copy %d split %d ray_dbl %d",
         L.scap, L.slog2, L.lcap, L.hcap, L.hlog2, L.hlcap, L.rec_bytes, L.sort_from, (int)L.sort_copy, (int)L.split,
         L.ray_dbl);
  for (int k = 0; k < LB_COUNT; k++)
    printf(" off_%s %zu size_%s %zu present_%s %d", BATCH_BUF_NAMES[k], L.off[k], BATCH_BUF_NAMES[k], L.size[k],
           BATCH_BUF_NAMES[k], (int)L.present[k]);
  printf(" set %zu tail %zu total %zu\n", L.set, L.tail, L.total);
  return 0;
}

// The cases: the arguments, one case each, or without arguments the lines of stdin.
static int buffers(int n, char** cases) {
  int rc = 0;
  for (int k = 0; k < n && !rc; k++) rc = buffers_case(cases[k]);
  char line[1024];
  while (n == 0 && !rc && fgets(line, sizeof line, stdin))
    if (line[strspn(line, " \t\r\n")]) rc = buffers_case(line);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s world.yml [sah] | --plan world.yml... | --buffers [case...]\n", argv[0]);
    return 2;
  }
  if (!strcmp(argv[1], "--plan")) return plans(argc - 2, argv + 2);
  if (!strcmp(argv[1], "--buffers")) return buffers(argc - 2, argv + 2);
  rtxcli::Scene sc;
  rtxcli::load_world(argv[1], sc);
  HostScene H;
  std::string msg;
  const rtx_status st = build_host_scene(&sc.desc, argc < 3 || argv[2][0] != '0', H, msg);
  if (st != RTX_OK) {
    printf("status %d %s\n", (int)st, msg.c_str());
    return 1;
  }
  array("runs", H.runs), array("sph64", H.sph64), array("sph32", H.sph32), array("planes", H.planes);
  array("boxes", H.boxes), array("mat", H.mat), array("bvh", H.bb->nodes), array("bvh_sph32", H.bb->slot32);
  array("bvh_sph64", H.bb->slot64), array("bvh_q", H.ql.rec), array("bvh_obj", H.bb->slot_obj);
  array("sph_obj", H.sph_obj), array("light", H.lights), array("tex", H.tex), array("texels", H.texels);
  array("lbuf", H.lb.words), array("rbuf", H.rb.words), array("rgate", H.gates);
  const SceneDev& S = H.dev;
#define I(f) printf("scalar " #f " %d\n", (int)S.f)
#define F(f) printf("scalar " #f " %a\n", (double)S.f)
  I(n_obj), I(n_light), I(n_sphere), I(n_plane), I(n_box), I(n_runs), I(n_nodes), I(n_slots), I(bvh_root), I(bvh_stack);
  F(max_distance), F(sse), F(sph_scale), I(sse_is_two);
  F(q_org[0]), F(q_org[1]), F(q_org[2]), F(q_step[0]), F(q_step[1]), F(q_step[2]), F(q_rstep), I(q_ok), F(q_err);
  F(root_c[0]), F(root_c[1]), F(root_c[2]), F(root_h[0]), F(root_h[1]), F(root_h[2]);
  I(lbuf_n), I(lbuf_stride), I(rbuf_n), I(rbuf_stride), I(rgate_stride), I(rbuf_sphere), F(rbuf_inv_m);
  return 0;
}
