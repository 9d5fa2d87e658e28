// Host-only check of the light buffer (tests/test_lbuf.py). stdin: "light x y z"
// lines, then "x y z r" sphere lines.  Packs the spheres and builds the hierarchy with
// rtx_scene_upload's own steps (rtx_scene_build.h) and the light buffer (build_light_buffer, cells per
// face side argv[1]), then for argv[2] random shadow-ray targets T per light (in and around the
// spheres' box, on and just off the spheres' surfaces, next to the light) finds every sphere within R
// of the segment [T, L] in binary64 (a superset of the spheres whose cover the reference counts) and
// checks that its leaf is listed in the cell the device looks up (query_lbuf's float32 arithmetic,
// restated below).  Prints the number of targets, of covering spheres and of misses (must be 0).
//
// Raise mode (argv[3] = "raise", argv[4] = the raise buffer's cells per face side; lights given as
// "light x y z radius"): builds the raise buffer at upload's floors (raise_floors) and, for argv[2]
// targets per light, places a random sphere exactly at a tangency of World#lit_area's acos raise
// (sphere.rb:42: d = |R - r1|, regime A or B, with a random axis through the light), rounds the target
// to binary64, checks in binary64 that it lies within 1e-9 S of the tangency, and counts those whose
// leaf is in none of the device's lists (the light buffer's cell, the raise buffer's B2 / B1 / M lists,
// lbuf_lookup.h shadow_lists) unless the device would walk the hierarchy for that target.  Prints the
// tangencies tested, the hierarchy fallbacks and the misses (must be 0).
//
// Upload mode (argv[1] = "upload", argv[2] = a world YAML, argv[3] = targets per light, argv[4] =
// "raise" for the raise check): the checks against the very buffers, gate blocks and floors
// build_host_scene makes for that world, which rtx_scene_upload ships.  Built only with
// -DLBUF_CHECK_UPLOAD, which takes the CLI's YAML loader in and so needs -lz.
#include <math.h>
#include <stdio.h>

#include <iostream>
#include <random>
#include <string>

#ifdef LBUF_CHECK_UPLOAD
#include "../raytracing_rb_amd/cli/scene_load.hpp"
#endif
#include "../raytracing_rb_amd/csrc/rtx_scene_build.h"
#include "lbuf_lookup.h"

using namespace rtx;

namespace {

using lbuf_host::device_cell;

// distance from C to the segment [A, B] (binary64)
double seg_dist(const double A[3], const double B[3], const double C[3]) {
  double ab[3], ac[3];
  for (int a = 0; a < 3; a++) ab[a] = B[a] - A[a], ac[a] = C[a] - A[a];
  const double dd = ab[0] * ab[0] + ab[1] * ab[1] + ab[2] * ab[2];
  double t = dd > 0 ? (ac[0] * ab[0] + ac[1] * ab[1] + ac[2] * ab[2]) / dd : 0.0;
  t = std::min(1.0, std::max(0.0, t));
  double e = 0.0;
  for (int a = 0; a < 3; a++) {
    const double q = A[a] + t * ab[a] - C[a];
    e += q * q;
  }
  return sqrt(e);
}

// sphere record -> its leaf reference / its slot
void sphere_places(const HostScene& H, std::vector<int32_t>& leaf_of, std::vector<int32_t>& slot_of) {
  const Bvh4Builder& bb = *H.bb;
  std::vector<int32_t> rec_of_obj(H.mat.size(), -1);
  for (size_t k = 0; k < H.sph_obj.size(); k++) rec_of_obj[(size_t)H.sph_obj[k]] = (int32_t)k;
  leaf_of.assign(H.sph64.size(), BVH_NONE);
  slot_of.assign(H.sph64.size(), -1);
  for (size_t k = 0; k < bb.slot_obj.size(); k++)
    if (bb.slot_obj[k] >= 0) slot_of[(size_t)rec_of_obj[(size_t)bb.slot_obj[k]]] = (int32_t)k;
  for (int32_t ref : leaf_refs(bb, H.dev.bvh_root)) {
    const int v = ~ref, slot0 = (v >> 2) * BVH_LEAF, cnt = (v & 3) + 1;
    for (int u = 0; u < cnt; u++)
      if (bb.slot_obj[(size_t)slot0 + u] >= 0) leaf_of[(size_t)rec_of_obj[(size_t)bb.slot_obj[(size_t)slot0 + u]]] = ref;
  }
}

int cover_check(const HostScene& H, int per_light) {
  const int n = H.lb.n, nl = H.dev.n_light;
  std::vector<int32_t> leaf_of, slot_of;
  sphere_places(H, leaf_of, slot_of);
  double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (const Sphere64& s : H.sph64)
    for (int a = 0; a < 3; a++) lo[a] = std::min(lo[a], s.c[a] - s.r), hi[a] = std::max(hi[a], s.c[a] + s.r);
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  long targets = 0, covers = 0, misses = 0, listed = 0;
  for (int li = 0; li < nl; li++) {
    const double* L = &H.lpos[3 * li];
    const uint16_t* blk = H.lb.words.data() + (size_t)H.lb.stride * li;
    const uint16_t* ent = blk + 6 * n * n + 1;
    for (int k = 0; k < per_light; k++) {
      double T[3];
      const int kind = k % 4;
      if (kind == 0 || H.sph64.empty()) {                 // the box and around it
        for (int a = 0; a < 3; a++) {
          const double w = hi[a] - lo[a] + 1.0;
          T[a] = lo[a] - 0.5 * w + 2.0 * w * U(rng);
        }
      } else if (kind <= 2) {                         // on or just off a sphere (shading targets)
        const Sphere64& s = H.sph64[(size_t)(U(rng) * H.sph64.size()) % H.sph64.size()];
        double u[3], r2 = 0;
        do {
          r2 = 0;
          for (int a = 0; a < 3; a++) u[a] = 2 * U(rng) - 1, r2 += u[a] * u[a];
        } while (r2 > 1 || r2 < 1e-6);
        const double off = kind == 1 ? 1e-5 : (U(rng) - 0.5) * 1e-3;
        for (int a = 0; a < 3; a++) T[a] = s.c[a] + u[a] / sqrt(r2) * (s.r + off);
      } else {                                        // near the light
        for (int a = 0; a < 3; a++) T[a] = L[a] + (2 * U(rng) - 1) * 0.5;
      }
      const double d[3] = {L[0] - T[0], L[1] - T[1], L[2] - T[2]};
      // the device's float images: d = L - T rounded, v = -d
      const int cell = device_cell(-(float)d[0], -(float)d[1], -(float)d[2], n);
      if (cell < 0) continue;                         // (the device walks the hierarchy)
      targets++;
      listed += blk[cell + 1] - blk[cell];
      for (size_t si = 0; si < H.sph64.size(); si++) {
        if (!(seg_dist(T, L, H.sph64[si].c) <= H.sph64[si].r * (1 + 1e-9))) continue;
        covers++;
        bool found = false;
        for (int e = blk[cell]; e < blk[cell + 1] && !found; e++) found = (int32_t)(int16_t)ent[e] == leaf_of[si];
        if (!found) {
          misses++;
          if (misses < 10)
            fprintf(stderr, "miss: light %d T (%.17g %.17g %.17g) sphere %zu cell %d\n", li, T[0], T[1], T[2], si, cell);
        }
      }
    }
  }
  printf("n %d targets %ld covers %ld misses %ld words %zu listed_x100 %ld\n", n, targets, covers, misses,
         (size_t)H.lb.stride * nl, targets ? 100 * listed / targets : 0);
  return misses ? 3 : 0;
}

// ------------------------------------------------------------------ raise mode
int raise_check(const HostScene& H, int per_light) {
  const int nl = H.dev.n_light;
  const bool per_sphere = H.dev.rbuf_sphere != 0;
  if (!H.lb.n || !H.rb.n || H.lb.n % H.rb.n) {
    printf("no buffers\n");
    return 1;
  }
  std::vector<int32_t> leaf_of, slot_of;
  sphere_places(H, leaf_of, slot_of);
  std::mt19937_64 rng(777);
  std::uniform_real_distribution<double> U(0.0, 1.0);
  long tested = 0, fallback = 0, misses = 0, listed = 0;
  for (int li = 0; li < nl; li++) {
    const double* L = &H.lpos[3 * li];
    const double rad = H.lrad[li];
    if (!(rad > 0.0)) continue;
    for (int k = 0; k < per_light; k++) {
      const size_t si = (size_t)(U(rng) * H.sph64.size()) % H.sph64.size();
      const Sphere64& sp = H.sph64[si];
      double u[3], r2;
      do {
        r2 = 0;
        for (int a = 0; a < 3; a++) u[a] = 2 * U(rng) - 1, r2 += u[a] * u[a];
      } while (r2 > 1 || r2 < 1e-6);
      for (int a = 0; a < 3; a++) u[a] /= sqrt(r2);
      // bias half the axes towards the sphere (its projection lands near the center)
      if (k % 2) {
        double w[3], wn = 0;
        for (int a = 0; a < 3; a++) w[a] = sp.c[a] - L[a], wn += w[a] * w[a];
        wn = sqrt(wn);
        const double spread = (sp.r + rad) / wn * 1.5 * U(rng);
        double un = 0;
        for (int a = 0; a < 3; a++) u[a] = w[a] / wn + spread * u[a], un += u[a] * u[a];
        for (int a = 0; a < 3; a++) u[a] /= sqrt(un);
      }
      double mu = 0;
      for (int a = 0; a < 3; a++) mu += (sp.c[a] - L[a]) * u[a];
      double dd = 0;
      for (int a = 0; a < 3; a++) {
        const double q = sp.c[a] - L[a] - mu * u[a];
        dd += q * q;
      }
      const double d = sqrt(dd);
      const bool regA = (k / 2) % 2 == 0;
      if (regA && !(d < sp.r)) continue;
      const double c = regA ? (sp.r - d) / rad : (sp.r + d) / rad;
      const double t = (k / 4) % 2 == 0 || fabs(1.0 - c) < 1e-6 ? mu / (1.0 + c) : mu / (1.0 - c);
      double T[3];
      for (int a = 0; a < 3; a++) T[a] = L[a] + t * u[a];
      // the reference's quantities in binary64 at the rounded target
      double lt[3], ctv[3], ltn2 = 0, dot = 0;
      for (int a = 0; a < 3; a++) lt[a] = L[a] - T[a], ctv[a] = sp.c[a] - T[a], ltn2 += lt[a] * lt[a], dot += ctv[a] * lt[a];
      const double tt = dot / ltn2;
      double x1t = 0, x1c = 0;
      for (int a = 0; a < 3; a++) {
        const double x1 = T[a] + lt[a] * tt;
        x1t += (x1 - T[a]) * (x1 - T[a]);
        x1c += (x1 - sp.c[a]) * (x1 - sp.c[a]);
      }
      const double r1 = rad * (sqrt(x1t) / sqrt(ltn2)), dd1 = sqrt(x1c);
      const double scale = fabs(L[0]) + fabs(L[1]) + fabs(L[2]) + fabs(sp.c[0]) + fabs(sp.c[1]) + fabs(sp.c[2]) + sp.r;
      if (!(fabs(dd1 - fabs(sp.r - r1)) <= 1e-9 * scale) || !(sqrt(ltn2) > 0)) continue;   // (not near a tangency)
      tested++;
      // the gate block as the device reads it: the cells' gates from word 8, the floats the light carries
      const lbuf_host::Lists ls = lbuf_host::shadow_lists(H.lb.words.data() + (size_t)H.lb.stride * li, H.lb.n,
                                                          H.rb.words.data() + (size_t)H.rb.stride * li,
                                                          H.gates.data() + (size_t)H.dev.rgate_stride * li + 8, H.rb.n, lt,
                                                          H.lights[li].raise_f2, H.lights[li].raise_lf2, per_sphere);
      if (ls.fallback) {
        fallback++;
        continue;
      }
      bool found = false;
      for (const auto* v : {&ls.cover, &ls.b2, &ls.b1, &ls.m}) {
        listed += v->size();
        const bool slots = per_sphere && v != &ls.cover;
        for (int32_t r : *v) found = found || r == (slots ? slot_of[si] : leaf_of[si]);
      }
      if (!found) {
        misses++;
        if (misses < 10)
          fprintf(stderr, "raise miss: light %d T (%.17g %.17g %.17g) sphere %zu regime %c t %.6g\n", li, T[0], T[1],
                  T[2], si, regA ? 'A' : 'B', t);
      }
    }
  }
  printf("n %d nc %d per_sphere %d tangencies %ld fallbacks %ld misses %ld rbuf_words %d listed_x100 %ld\n", H.lb.n, H.rb.n,
         (int)per_sphere, tested, fallback, misses, H.rb.stride, tested ? 100 * listed / std::max(1L, tested - fallback) : 0);
  return misses ? 3 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  HostScene H;
  std::string msg;
#ifdef LBUF_CHECK_UPLOAD
  if (argc > 2 && std::string(argv[1]) == "upload") {
    rtxcli::Scene sc;
    rtxcli::load_world(argv[2], sc);
    if (build_host_scene(&sc.desc, true, H, msg) != RTX_OK || !H.lb.n) {
      printf("no light buffer %s\n", msg.c_str());
      return 1;
    }
    const int per_light = argc > 3 ? atoi(argv[3]) : 20000;
    return argc > 4 && std::string(argv[4]) == "raise" ? raise_check(H, per_light) : cover_check(H, per_light);
  }
#endif
  const int n = argc > 1 ? atoi(argv[1]) : 16;
  const int per_light = argc > 2 ? atoi(argv[2]) : 100000;
  const bool raise_mode = argc > 3 && std::string(argv[3]) == "raise";
  const int nc = argc > 4 ? atoi(argv[4]) : 8;
  std::vector<rtx_object_desc> objs;
  std::vector<rtx_light_desc> lights;
  std::string tok;
  while (std::cin >> tok) {
    if (tok == "light") {
      rtx_light_desc l{};
      std::cin >> l.position[0] >> l.position[1] >> l.position[2];
      if (raise_mode) std::cin >> l.radius;
      lights.push_back(l);
      continue;
    }
    rtx_object_desc o{};
    o.type = RTX_SPHERE;
    o.texture_id = -1;
    o.has_refractive_rate = 1;
    o.center[0] = std::stod(tok);
    std::cin >> o.center[1] >> o.center[2] >> o.radius;
    objs.push_back(o);
  }
  rtx_scene_desc sd{};
  sd.n_objects = (int32_t)objs.size(), sd.objects = objs.data();
  sd.n_lights = (int32_t)lights.size(), sd.lights = lights.data();
  if (pack_objects(&sd, H, msg) != RTX_OK) {
    printf("bad scene %s\n", msg.c_str());
    return 1;
  }
  build_hierarchy(H, true);
  pack_lights(&sd, H);
  H.lb = build_light_buffer(*H.bb, H.dev.bvh_root, H.light_pos(), sd.n_lights, n, 1u << 30,
                            raise_mode ? H.lrad.data() : nullptr);
  if (!H.lb.n) {
    printf("no light buffer\n");
    return 1;
  }
  if (!raise_mode) return cover_check(H, per_light);
  H.lfloor = raise_floors(&sd);
  H.dev.rbuf_sphere = small_scene(H) ? 0 : 1;          // (rtx_scene_upload's choice)
  H.rb = build_raise_buffer(*H.bb, H.dev.bvh_root, H.light_pos(), H.lrad.data(), H.lfloor.data(), sd.n_lights, nc,
                            (size_t)1 << 30, H.dev.rbuf_sphere != 0);
  pack_gates(H);
  return raise_check(H, per_light);
}
