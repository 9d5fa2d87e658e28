// walk_sim.cpp — CPU simulator of librtx's hierarchy walks (analysis tool; not
// product code, not the oracle).  It loads a scene with the native CLI's YAML
// loader, builds the scene with the library's own host scene build (csrc/rtx_scene_build.h: the
// records, tree, buffers and floors of rtx_scene_upload), traces the camera's ray trees in binary64
// (approximate shading: the ray distribution, not the pixels, is what matters
// here) and, for every shadow ray of World#local_lights, counts the work of the
// shadow walk under several culling rules:
//
//   seg       the segment walk (child boxes dilated by m S, t in [0, 1]):
//             the exact_raises = 0 walk;
//   cyl_sym   exact_raises as first built (r09b): boxes dilated by radius tm + mg
//             over t in [-tm, tm], one bound tm for both nappes of the cone;
//   cyl_asym  the same with each nappe's own bound: t in [-tb, tf], dilation
//             radius max(tb, tf) + mg;
//   cone_box  per child box its own dilation radius max|t| + mg (t over the
//             box's projection on the axis), t in [-tb, tf];
//   cone      the exact L-infinity cone test per child box (both nappes).
//
// Counts per shadow walk: inner nodes visited, child boxes tested, leaves
// visited, spheres pre-tested, spheres the raise band keeps.  The nearest-hit
// walks are counted too (seg rule with the shrinking far bound).
//
//   g++ -O2 -std=c++17 -o tools/walk_sim tools/walk_sim.cpp -lz
//   tools/walk_sim scenes/c2_world.yml scenes/c2_camera.yml [stride] [max_rays_per_level]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../raytracing_rb_amd/cli/scene_load.hpp"
#include "../raytracing_rb_amd/csrc/rtx_scene_build.h"
#include "lbuf_lookup.h"

using namespace rtx;

namespace {

// The scene as rtx_scene_upload builds it, plus the description's objects and lights (binary64 geometry).
struct Sim : HostScene {
  std::vector<rtx_object_desc> obj;
  std::vector<rtx_light_desc> lights;   // (hides HostScene::lights, the device records)
  bool q16 = false;
  double maxd = 1e4;

  void build(const rtx_scene_desc& sd, bool sah) {
    obj.assign(sd.objects, sd.objects + sd.n_objects);
    lights.assign(sd.lights, sd.lights + sd.n_lights);
    maxd = sd.max_distance;
    std::string msg;
    if (pack_objects(&sd, *this, msg) != RTX_OK) {
      fprintf(stderr, "%s\n", msg.c_str());
      exit(1);
    }
    // (the library's rule: the median tree when only it fits LDS; WAVE_SIM_TREE=median / sah forces one)
    const char* force = getenv("WAVE_SIM_TREE");
    build_hierarchy(*this, sah && !(force && !strcmp(force, "median")), !force);
    if (const char* qb = getenv("WAVE_SIM_QUANT")) {   // child boxes on an 2^bits grid over the node's own box, rounded out
      const float steps = (float)((1 << atoi(qb)) - 1);
      for (Bvh4Node& n : bb->nodes)
        for (int a = 0; a < 3; a++) {
          float lo = INFINITY, hi = -INFINITY;
          for (int k = 0; k < 4; k++)
            if (n.child[k] != BVH_NONE) lo = fminf(lo, n.lh[a][k][0]), hi = fmaxf(hi, n.lh[a][k][1]);
          const float ext = (hi - lo) / steps;
          if (!(ext > 0)) continue;
          for (int k = 0; k < 4; k++) {
            if (n.child[k] == BVH_NONE) continue;
            n.lh[a][k][0] = lo + floorf((n.lh[a][k][0] - lo) / ext) * ext;
            n.lh[a][k][1] = fminf(hi, lo + ceilf((n.lh[a][k][1] - lo) / ext) * ext);
          }
        }
    }
    pack_quantized_leaves(*this);
    q16 = ql.ok && sph64.size() > 256;        // C4-sized scenes run SPH_BVH_QLDS
    sphere_box(*this);
  }
};

// ------------------------------------------------------------------ exact geometry (binary64)
bool sphere_hit(const Sphere64& s, V3 o, V3 d, double& t_out, bool& inside) {
  const V3 C = v3p(s.c);
  const V3 oc = vsub(C, o);
  const double dd = vdot(d, d);
  const double t = vdot(oc, d) / dd;
  const V3 np = vadd(o, vsc(d, t));
  const double nd = vr(vsub(np, C));
  if (!(nd <= s.r)) return false;
  const double h = sqrt(s.r * s.r - nd * nd) / sqrt(dd);
  inside = vr(oc) <= s.r;
  const double th = inside ? t + h : t - h;
  if (!inside && t < 0) return false;
  if (th < 0) return false;
  t_out = th;
  return true;
}

bool plane_hit(const rtx_object_desc& p, V3 o, V3 d, double& t) {
  const V3 F = v3p(p.front);
  const double den = vdot(F, d);
  if (den == 0) return false;
  t = vdot(vsub(v3p(p.point), o), F) / den;
  return t >= 0;
}

// ------------------------------------------------------------------ walks
struct Stats {
  double walks = 0, nodes = 0, tests = 0, leaves = 0, spheres = 0, band = 0, band2 = 0, band3 = 0;
  void add(const Stats& o) {
    walks += o.walks, nodes += o.nodes, tests += o.tests, leaves += o.leaves, spheres += o.spheres, band += o.band;
    band2 += o.band2, band3 += o.band3;
  }
};

enum Rule { SEG = 0, CYL_SYM, CYL_ASYM, CONE_BOX, CONE, NRULE };
const char* rule_name[NRULE] = {"seg", "cyl_sym", "cyl_asym", "cone_box", "cone"};

struct RayF {
  float o[3], d[3], i[3], dd, Sx, mS;
};

RayF rayf(const Sim& S, V3 o, V3 d) {
  RayF r;
  r.o[0] = (float)o.x, r.o[1] = (float)o.y, r.o[2] = (float)o.z;
  r.d[0] = (float)d.x, r.d[1] = (float)d.y, r.d[2] = (float)d.z;
  r.dd = r.d[0] * r.d[0] + r.d[1] * r.d[1] + r.d[2] * r.d[2];
  r.Sx = fabsf(r.o[0]) + fabsf(r.o[1]) + fabsf(r.o[2]) + S.dev.sph_scale;
  r.mS = CULL_M * r.Sx;
  const float l1 = fabsf(r.d[0]) + fabsf(r.d[1]) + fabsf(r.d[2]), tiny = 1e-20f * l1;
  for (int a = 0; a < 3; a++) {
    const float e = fabsf(r.d[a]) < tiny ? copysignf(tiny, r.d[a]) : r.d[a];
    r.i[a] = 1.0f / e;
  }
  return r;
}

// slab test of box (lo, hi) dilated by dil over t in [tlo, thi]; entry t or inf
float slab(const RayF& r, const float lo[3], const float hi[3], float dil, float tlo, float thi) {
  float tn = -INFINITY, tf = INFINITY;
  for (int a = 0; a < 3; a++) {
    const float t0 = (lo[a] - dil - r.o[a]) * r.i[a], t1 = (hi[a] + dil - r.o[a]) * r.i[a];
    tn = fmaxf(tn, fminf(t0, t1));
    tf = fminf(tf, fmaxf(t0, t1));
  }
  return (tn <= tf && tf >= tlo && tn <= thi) ? tn : INFINITY;
}

// the exact L-infinity cone test: some t with Q(t) within rad |t| + mg of the box on every axis
bool cone_box_exact(const RayF& r, const float lo[3], const float hi[3], float rad, float mg) {
  for (int nap = 0; nap < 2; nap++) {          // nap 0: t >= 0, nap 1: t <= 0 (tau = -t >= 0)
    float lower = 0.0f, upper = INFINITY;
    bool ok = true;
    for (int a = 0; a < 3 && ok; a++) {
      const float da = nap ? -r.d[a] : r.d[a];
      // lo - mg - rad tau <= o + tau da <= hi + mg + rad tau
      const float L = lo[a] - mg - r.o[a], H = hi[a] + mg - r.o[a];
      const float p = da + rad, m = da - rad;  // tau p >= L, tau m <= H
      if (p > 0) lower = fmaxf(lower, L / p);
      else if (p < 0) upper = fminf(upper, L / p);
      else if (L > 0) ok = false;
      if (m > 0) upper = fminf(upper, H / m);
      else if (m < 0) lower = fmaxf(lower, H / m);
      else if (H < 0) ok = false;
    }
    if (ok && lower <= upper * (1 + 1e-5f) + 1e-30f) return true;
  }
  return false;
}

// nappe bounds of the cone against the spheres' box (t in [-tb, tf])
void nappe_bounds(const Sim& S, const RayF& r, float rad, float mg, float& tb, float& tf, float& tm) {
  tb = tf = tm = INFINITY;
  for (int a = 0; a < 3; a++) {
    const float ad = fabsf(r.d[a]), den = ad - rad;
    if (!(den > 1e-5f * (ad + rad))) continue;
    const float lo = S.dev.root_c[a] - S.dev.root_h[a], hi = S.dev.root_c[a] + S.dev.root_h[a];
    tm = fminf(tm, (S.dev.root_h[a] + mg + fabsf(S.dev.root_c[a] - r.o[a])) / den);
    const float up = (hi + mg - r.o[a]) / den, dn = (r.o[a] - lo + mg) / den;   // toward +a / -a
    if (r.d[a] > 0) tf = fminf(tf, up), tb = fminf(tb, dn);
    else tf = fminf(tf, dn), tb = fminf(tb, up);
  }
  tb = fmaxf(tb, 0.0f) * (1 + 1e-5f);
  tf = fmaxf(tf, 0.0f) * (1 + 1e-5f);
  tm *= 1 + 1e-5f;
}

// One shadow walk (T = o, d = L - T) under `rule`; the exact covers are not needed here.
Stats shadow_walk(const Sim& S, V3 o, V3 d, double radius, Rule rule) {
  Stats st;
  st.walks = 1;
  const RayF r = rayf(S, o, d);
  const float rad = (float)radius, D = sqrtf(r.dd);
  const float mg = CULL_M * r.Sx * (1.0f + rad / D) + (S.q16 ? (2.0f + rad / D) * S.dev.q_err : 0.0f);
  float tb, tf, tm;
  nappe_bounds(S, r, rad, mg, tb, tf, tm);
  float tlo = 0.0f, thi = 1.0f + 1e-5f + r.mS / D, dil = r.mS;
  if (rule == CYL_SYM) tlo = -tm, thi = tm, dil = rad * tm + mg;
  if (rule == CYL_ASYM || rule == CONE_BOX) tlo = -tb, thi = tf, dil = rad * std::max(tb, tf) + mg;
  if (rule != SEG && !(std::isfinite(tm) && std::isfinite(tb) && std::isfinite(tf))) {   // every sphere
    st.spheres = (double)S.sph64.size();
    st.band = st.spheres;
    return st;
  }
  const float kq = rad / r.dd;
  // the band's own tolerance: 32 float32 ulps of the scene scale (the float32
  // geometry's error is below 10), + the 16-bit records' decoding error
  const float mgb = 32.0f * 5.96e-8f * r.Sx * (1.0f + rad / D);
  const float mgq = mgb + (S.q16 ? (2.0f + rad / D) * S.dev.q_err : 0.0f);
  std::vector<int> stk;
  if (S.dev.bvh_root == BVH_NONE) return st;
  stk.push_back(S.dev.bvh_root);
  while (!stk.empty()) {
    const int ref = stk.back();
    stk.pop_back();
    if (ref >= 0) {
      st.nodes++;
      const Bvh4Node& n = S.bb->nodes[ref];
      for (int k = 0; k < 4; k++) {
        if (n.child[k] == BVH_NONE) continue;
        st.tests++;
        const float lo[3] = {n.lh[0][k][0], n.lh[1][k][0], n.lh[2][k][0]};
        const float hi[3] = {n.lh[0][k][1], n.lh[1][k][1], n.lh[2][k][1]};
        bool want;
        if (rule == CONE) {
          want = cone_box_exact(r, lo, hi, rad, mg) || slab(r, lo, hi, r.mS, 0.0f, 1.0f + 1e-5f + r.mS / D) < INFINITY;
        } else if (rule == CONE_BOX) {
          float t0 = 0.0f, t1 = 0.0f;          // the box's projection on the axis (in t)
          for (int a = 0; a < 3; a++) {
            const float p = (lo[a] - r.o[a]) * r.d[a] / r.dd, q = (hi[a] - r.o[a]) * r.d[a] / r.dd;
            t0 += fminf(p, q), t1 += fmaxf(p, q);
          }
          const float dl = rad * fmaxf(fabsf(t0), fabsf(t1)) + mg;
          want = slab(r, lo, hi, dl, tlo, thi) < INFINITY;
        } else {
          want = slab(r, lo, hi, dil, tlo, thi) < INFINITY;
        }
        if (want) stk.push_back(n.child[k]);
      }
    } else {
      st.leaves++;
      const int v = ~ref, slot0 = (v >> 2) * BVH_LEAF, cnt = (v & 3) + 1;
      for (int u = 0; u < cnt; u++) {
        st.spheres++;
        if (rule == SEG) continue;
        const float* c = &S.bb->slot32[(size_t)(v >> 2) * 16];
        const float ox = c[u] - r.o[0], oy = c[4 + u] - r.o[1], oz = c[8 + u] - r.o[2];
        const float sq = ox * ox + oy * oy + oz * oz, q = ox * r.d[0] + oy * r.d[1] + oz * r.d[2];
        const float l = sq * r.dd - q * q, R = sqrtf(c[12 + u]);
        const float t = fabsf(R - kq * fabsf(q));
        auto band = [&](float w) {
          const float lo = fmaxf(t - w, 0.0f), hi = t + w;
          const float e = 4e-6f * (sq + hi * hi) * r.dd;
          return l >= lo * lo * r.dd - e && l <= hi * hi * r.dd + e;
        };
        if (band(mg)) st.band++;             // (r09b's band: the box dilation's mg)
        if (band(mgq)) st.band2++;           // 32 ulps (+ the 16-bit decoding error)
        if (band(mgb)) st.band3++;           // 32 ulps on float32 records
      }
      (void)slot0;
    }
  }
  return st;
}

// nearest hit over every object (binary64; spheres through the hierarchy, counted)
int nearest(const Sim& S, V3 o, V3 d, double& best_t, bool& inside, Stats& st) {
  st.walks++;
  int besti = -1;
  best_t = INFINITY;
  for (size_t i = 0; i < S.obj.size(); i++) {
    if (S.obj[i].type != RTX_PLANE) continue;
    double t;
    if (plane_hit(S.obj[i], o, d, t) && t < best_t && vr(vsc(d, t)) < S.maxd) best_t = t, besti = (int)i, inside = false;
  }
  if (S.dev.bvh_root == BVH_NONE) return besti;
  const RayF r = rayf(S, o, d);
  std::vector<int> stk{S.dev.bvh_root};
  while (!stk.empty()) {
    const int ref = stk.back();
    stk.pop_back();
    const float thi = std::isfinite(best_t) ? (float)(best_t * (1 + 1e-6)) : INFINITY;
    if (ref >= 0) {
      st.nodes++;
      const Bvh4Node& n = S.bb->nodes[ref];
      for (int k = 0; k < 4; k++) {
        if (n.child[k] == BVH_NONE) continue;
        st.tests++;
        const float lo[3] = {n.lh[0][k][0], n.lh[1][k][0], n.lh[2][k][0]};
        const float hi[3] = {n.lh[0][k][1], n.lh[1][k][1], n.lh[2][k][1]};
        if (slab(r, lo, hi, r.mS, 0.0f, thi) < INFINITY) stk.push_back(n.child[k]);
      }
    } else {
      st.leaves++;
      const int v = ~ref, slot0 = (v >> 2) * BVH_LEAF, cnt = (v & 3) + 1;
      for (int u = 0; u < cnt; u++) {
        st.spheres++;
        double t;
        bool in;
        if (sphere_hit(S.bb->slot64[slot0 + u], o, d, t, in) && t < best_t) {
          best_t = t, besti = S.bb->slot_obj[slot0 + u], inside = in;
        }
      }
    }
  }
  return besti;
}

struct Ray {
  V3 o, d, att;
  int depth;
};

}  // namespace

#ifndef WALK_SIM_NO_MAIN
int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s world.yml camera.yml [stride] [max_rays_per_level]\n", argv[0]);
    return 2;
  }
  const int stride = argc > 3 ? atoi(argv[3]) : 8;
  const size_t cap = argc > 4 ? (size_t)atoll(argv[4]) : 200000;
  rtxcli::Scene sc;
  rtxcli::load_world(argv[1], sc);
  const rtx_camera_desc cam = rtxcli::load_camera(argv[2]);
  Sim S;
  S.build(sc.desc, true);
  printf("scene: %zu spheres, %zu nodes, %zu slots, stack %d, q16 %d, q_err %.3g, sph_scale %.3g\n", S.sph64.size(),
         S.bb->nodes.size(), S.bb->slot_obj.size(), S.bb->stack + 1, (int)S.q16, S.dev.q_err, S.dev.sph_scale);
  // the light buffer and the raise buffer as rtx_scene_upload chooses them; COVER_N / RAISE_N (cells per face
  // side) and PER_SPHERE (per-sphere raise lists) override its choice
  const int nl = (int)S.lights.size();
  pack_lights(&sc.desc, S);
  S.lfloor = raise_floors(&sc.desc);
  choose_light_buffer(S);
  if (getenv("COVER_N"))
    S.lb = build_light_buffer(*S.bb, S.dev.bvh_root, S.light_pos(), nl, atoi(getenv("COVER_N")), 1u << 30, S.lrad.data());
  if (getenv("RAISE_N") || getenv("PER_SPHERE")) {
    const int raise_n = getenv("RAISE_N") ? atoi(getenv("RAISE_N")) : (small_scene(S) ? 12 : RTX_RBUF_GLOBAL_N);
    S.dev.rbuf_sphere = getenv("PER_SPHERE") != nullptr;
    S.rb = build_raise_buffer(*S.bb, S.dev.bvh_root, S.light_pos(), S.lrad.data(), S.lfloor.data(), nl, raise_n,
                              (size_t)1 << 30, S.dev.rbuf_sphere != 0);
  } else {
    choose_raise_buffer(S);
  }
  pack_gates(S);
  const bool per_sphere = S.dev.rbuf_sphere != 0;
  printf("light buffer n %d: %d words per light; raise buffer n %d: %d words per light, floor %.4g (nearest surface "
         "%.4g), flags %d\n",
         S.lb.n, S.lb.stride, S.rb.n, S.rb.stride, S.rb.n ? raise_floor(S.rb, 0) : 0.0, S.lfloor[0] / 0.99, 1);
  double rs_walks = 0, rs_cover = 0, rs_p = 0, rs_m = 0, rs_fb = 0, rs_union = 0, rs_band = 0, rs_scan = 0, rs_lookups = 0;
  std::vector<int> scan_hist, need_b2, need_b1, need_m;   // per shadow walk (raise-list entries read / needed)
  std::vector<std::vector<int32_t>> cover_seq;      // per shadow walk: the light buffer's cell
  // camera rays (pinhole through the pixel centers of every stride-th pixel; lens jitter ignored)
  const V3 pos = v3p(cam.position), front = v3p(cam.front), up = v3p(cam.up);
  uint32_t e = 0;
  const V3 left = vnorm(vcross(up, front), e), upn = vnorm(up, e), fn = vnorm(front, e);
  std::vector<Ray> level;
  for (int y = 0; y < cam.height; y += stride)
    for (int x = 0; x < cam.width; x += stride) {
      const double u = 2.0 * ((double)x / cam.width - 0.5) * cam.retina_width;
      const double w = 2.0 * ((double)y / cam.height - 0.5) * cam.retina_height;
      const V3 dir = vadd(vsc(fn, cam.image_distance), vadd(vsc(left, -u), vsc(upn, -w)));
      level.push_back(Ray{pos, dir, v3(1, 1, 1), cam.trace_depth});
    }
  std::mt19937_64 rng(1);
  Stats tot_sh[NRULE], tot_ext;
  double child_hist[8] = {0};                     // parents (hits above the last level) by children
  for (int lev = 0; lev < cam.trace_depth && !level.empty(); lev++) {
    if (level.size() > cap) {                   // a uniform subsample of the level
      std::vector<Ray> sub;
      const double step = (double)level.size() / cap;
      for (size_t k = 0; k < cap; k++) sub.push_back(level[(size_t)(k * step)]);
      level.swap(sub);
    }
    Stats sh[NRULE], ext;
    size_t hits = 0;
    std::vector<Ray> next;
    for (const Ray& ray : level) {
      double t;
      bool inside = false;
      const int oi = nearest(S, ray.o, ray.d, t, inside, ext);
      if (oi < 0) continue;
      hits++;
      const rtx_object_desc& ob = S.obj[oi];
      const V3 hit = vadd(ray.o, vsc(ray.d, t));
      V3 n, delta;
      if (ob.type == RTX_SPHERE) {
        const V3 C = v3p(ob.center);
        n = inside ? vsub(C, hit) : vsub(hit, C);
        delta = vsc(vsub(hit, C), 1e-5 * (inside ? -1.0 : 1.0));
      } else {
        n = v3p(ob.front);
        if (vdot(n, ray.d) > 0) n = vneg(n);
        delta = vsc(n, 1e-5);
      }
      const V3 T = vadd(hit, delta);
      int nl = 0;
      for (const rtx_light_desc& L : S.lights) {
        const V3 lt = vsub(v3p(L.position), T);
        for (int rr = 0; rr < NRULE; rr++) sh[rr].add(shadow_walk(S, T, lt, L.radius, (Rule)rr));
        {                                            // light buffer / raise buffer lookups
          const int li = (int)(&L - S.lights.data());
          const double dl[3] = {lt.x, lt.y, lt.z};
          rs_walks++;
          if (S.lb.n && S.rb.n) {
            const LightDev& ld = S.HostScene::lights[li];   // (the gates and floats as the device reads them)
            const lbuf_host::Lists ls = lbuf_host::shadow_lists(
                S.lb.words.data() + (size_t)S.lb.stride * li, S.lb.n, S.rb.words.data() + (size_t)S.rb.stride * li,
                S.gates.data() + (size_t)S.dev.rgate_stride * li + 8, S.rb.n, dl, ld.raise_f2, ld.raise_lf2, per_sphere);
            if (ls.fallback) {
              rs_fb++;
            } else {
              rs_cover += ls.cover.size();
              rs_p += ls.b2.size() + ls.b1.size();
              rs_m += ls.m.size();
              rs_scan += ls.scanned;
              std::vector<int32_t> un = ls.cover;
              for (const auto* v : {&ls.b2, &ls.b1, &ls.m}) un.insert(un.end(), v->begin(), v->end());
              if (per_sphere) {
                for (int32_t r : ls.cover) rs_band += ((~r) & 3) + 1;
                rs_band += ls.b2.size() + ls.b1.size() + ls.m.size();
                un = ls.cover;
              } else {
                for (int32_t r : un) rs_band += ((~r) & 3) + 1;
              }
              std::sort(un.begin(), un.end());
              rs_union += std::unique(un.begin(), un.end()) - un.begin();
              rs_lookups += (ls.scanned > 0);
              scan_hist.push_back(ls.scanned);
              cover_seq.push_back(ls.cover);
              need_b2.push_back((int)ls.b2.size()), need_b1.push_back((int)ls.b1.size()), need_m.push_back((int)ls.m.size());
            }
          }
        }
        // lit unless a sphere or plane crosses the segment (approximate local_lights)
        bool blocked = false;
        for (size_t i = 0; i < S.obj.size() && !blocked; i++) {
          double tt;
          bool in;
          if (S.obj[i].type == RTX_SPHERE) {
            Sphere64 s;
            for (int a = 0; a < 3; a++) s.c[a] = S.obj[i].center[a];
            s.r = S.obj[i].radius;
            if (S.sph64.size() > 256) continue;     // (C4: skip the brute-force occlusion estimate)
            blocked = sphere_hit(s, T, lt, tt, in) && tt < 1.0;
          }
        }
        if (!blocked) nl++;
      }
      if (ray.depth - 1 <= 0) continue;
      const size_t nch0 = next.size();
      struct ChildCount {
        std::vector<Ray>& nx;
        size_t n0;
        double* h;
        ~ChildCount() { h[std::min<size_t>(nx.size() - n0, 7)]++; }   // (the parent's child block size)
      } cc_{next, nch0, child_hist};
      const V3 nn = vnorm(n, e);
      const V3 dn = vnorm(ray.d, e);
      const V3 ra = vmul(ray.att, v3p(ob.reflective_attenuation));
      if (vr(ra) >= 1e-4) {
        const V3 rd = vsub(dn, vsc(nn, 2.0 * vdot(dn, nn)));
        next.push_back(Ray{T, rd, ra, ray.depth - 1});
      }
      const V3 fa = vmul(ray.att, v3p(ob.refractive_attenuation));
      if (ob.type == RTX_SPHERE && vr(fa) >= 1e-4) {
        const double eta = inside ? ob.refractive_rate : 1.0 / ob.refractive_rate;
        const double ci = -vdot(dn, nn), k = 1 - eta * eta * (1 - ci * ci);
        if (k >= 0) {
          const V3 td = vadd(vsc(dn, eta), vsc(nn, eta * ci - sqrt(k)));
          next.push_back(Ray{vsub(hit, vsc(nn, 1e-5)), td, fa, ray.depth - 1});
        }
      }
      if (nl == 0 && cam.monte_carlo_diffusion_times > 0) {
        std::uniform_real_distribution<double> U(0, 1);
        for (int k = 0; k < cam.monte_carlo_diffusion_times; k++) {
          V3 dir = v3(U(rng) - 0.5, U(rng) - 0.5, U(rng) - 0.5);
          if (vdot(dir, nn) < 0) dir = vneg(dir);
          const V3 pa = vmul(ray.att, vsc(v3p(ob.diffuse_rate), 1.0 / cam.monte_carlo_diffusion_times));
          if (vr(pa) >= 1e-4) next.push_back(Ray{T, dir, pa, ray.depth - 1});
        }
      }
    }
    printf("level %d: rays %zu, hits %zu\n", lev, level.size(), hits);
    printf("  extend   per walk: nodes %6.2f tests %6.2f leaves %6.2f spheres %6.2f\n", ext.nodes / ext.walks,
           ext.tests / ext.walks, ext.leaves / ext.walks, ext.spheres / ext.walks);
    for (int rr = 0; rr < NRULE; rr++)
      printf("  %-8s per walk: nodes %6.2f tests %6.2f leaves %6.2f spheres %6.2f band %8.5f\n", rule_name[rr],
             sh[rr].nodes / sh[rr].walks, sh[rr].tests / sh[rr].walks, sh[rr].leaves / sh[rr].walks,
             sh[rr].spheres / sh[rr].walks, sh[rr].band / sh[rr].walks);
    for (int rr = 0; rr < NRULE; rr++) tot_sh[rr].add(sh[rr]);
    tot_ext.add(ext);
    level.swap(next);
  }
  printf("all levels:\n  extend   per walk: nodes %6.2f tests %6.2f leaves %6.2f spheres %6.2f\n",
         tot_ext.nodes / tot_ext.walks, tot_ext.tests / tot_ext.walks, tot_ext.leaves / tot_ext.walks,
         tot_ext.spheres / tot_ext.walks);
  for (int rr = 0; rr < NRULE; rr++)
    printf("  %-8s per walk: nodes %6.2f tests %6.2f leaves %6.2f spheres %6.2f band %8.5f %8.5f %8.5f (x seg leaves %.2f)\n",
           rule_name[rr], tot_sh[rr].nodes / tot_sh[rr].walks, tot_sh[rr].tests / tot_sh[rr].walks,
           tot_sh[rr].leaves / tot_sh[rr].walks, tot_sh[rr].spheres / tot_sh[rr].walks,
           tot_sh[rr].band / tot_sh[rr].walks, tot_sh[rr].band2 / tot_sh[rr].walks, tot_sh[rr].band3 / tot_sh[rr].walks,
           tot_sh[rr].leaves / tot_sh[SEG].leaves);
  {
    // k_tree_finalize's reads: 32-B tree records, a parent's
    // children contiguous; 64-B segments its child block touches, at a random
    // 32-B alignment (today) and with each block 64-B aligned
    double parents = 0, kids = 0, seg_now = 0, seg_al = 0;
    for (int k = 1; k < 8; k++) {
      parents += child_hist[k], kids += k * child_hist[k];
      seg_now += child_hist[k] * (k + 1) / 2.0;   // (k + 1) / 2 on average over both parities
      seg_al += child_hist[k] * ((k + 1) / 2);
    }
    printf("tree records: parents by children:");
    for (int k = 0; k < 8; k++) printf(" %d:%.0f", k, child_hist[k]);
    printf("\n  child blocks %.0f, records %.0f, 64-B segments %.0f now, %.0f aligned (%.1f %% fewer)\n", parents, kids,
           seg_now, seg_al, 100.0 * (1.0 - seg_al / std::max(1.0, seg_now)));
  }
  if (!scan_hist.empty()) {
    // the tail: a wave runs its lanes' list loops to the longest one
    auto pct = [](std::vector<int> v, double p) { std::sort(v.begin(), v.end()); return v[(size_t)(p * (v.size() - 1))]; };
    double mx64 = 0, n64 = 0;
    for (size_t k = 0; k + 64 <= scan_hist.size(); k += 64, n64++)
      mx64 += *std::max_element(scan_hist.begin() + k, scan_hist.begin() + k + 64);
    printf("raise entries read per walk: p50 %d p90 %d p99 %d max %d; mean of the max over 64 consecutive walks %.1f\n",
           pct(scan_hist, 0.5), pct(scan_hist, 0.9), pct(scan_hist, 0.99), pct(scan_hist, 1.0), mx64 / std::max(1.0, n64));
    printf("needed per walk p99: B2 %d B1 %d M %d; max B2 %d B1 %d M %d\n", pct(need_b2, 0.99), pct(need_b1, 0.99),
           pct(need_m, 0.99), pct(need_b2, 1.0), pct(need_b1, 1.0), pct(need_m, 1.0));
  }
  if (!cover_seq.empty()) {
    // a wave of 64 consecutive shadow walks: today each lane loops over its own cell's list (the wave
    // runs the longest); a union bitmask loops over the union of the 64 cells, uniformly
    double mean = 0, mx = 0, un = 0, n64 = 0;
    for (const auto& c : cover_seq) mean += c.size();
    for (size_t k = 0; k + 64 <= cover_seq.size(); k += 64, n64++) {
      std::vector<int32_t> u;
      size_t m = 0;
      for (size_t w = k; w < k + 64; w++) u.insert(u.end(), cover_seq[w].begin(), cover_seq[w].end()), m = std::max(m, cover_seq[w].size());
      std::sort(u.begin(), u.end());
      un += std::unique(u.begin(), u.end()) - u.begin();
      mx += m;
    }
    printf("cover cells per 64 consecutive shadow walks: mean list %.3f, longest list %.3f, union %.3f\n",
           mean / cover_seq.size(), mx / std::max(1.0, n64), un / std::max(1.0, n64));
  }
  printf("light/raise buffers per shadow walk: cover leaves %.3f, raise B2+B1 %.3f, raise M %.3f, distinct leaves %.3f, "
         "band spheres %.3f, raise entries read %.3f (walks with an open gate %.3f), hierarchy fallbacks %.5f\n",
         rs_cover / rs_walks, rs_p / rs_walks, rs_m / rs_walks, rs_union / rs_walks, rs_band / rs_walks, rs_scan / rs_walks,
         rs_lookups / rs_walks, rs_fb / rs_walks);
  return 0;
}
#endif  // WALK_SIM_NO_MAIN
