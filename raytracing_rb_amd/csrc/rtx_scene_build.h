// rtx_scene_build.h — host-only (no HIP calls, plain g++ -std=c++17): a scene description
// (include/rtx.h) turned into every array and scalar the device receives.  rtx_scene_upload
// (rtx_capi.cpp) builds a HostScene and copies it; the host tools (tools/scene_dump.cpp,
// lbuf_check.cpp, qleaf_check.cpp, walk_sim.cpp) build the same HostScene, or call single
// steps, so they see what upload ships.  Scene preparation restates the constructors of the
// reference (src/world.rb:15-34, src/objects/{sphere,plane,box,texture}.rb) with the same
// operation order, so every constant the device uses has the bits the Ruby code would compute.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <memory>
#include <string>

#include "../../include/rtx.h"
#include "rtx_bvh_build.h"
#include "rtx_vec3.h"

#ifndef RTX_LBUF_GLOBAL_N
#define RTX_LBUF_GLOBAL_N 160      // C4: 251 ms per frame against 253 ms with 128 and 256 ms with 96 (r10t)
#endif
#ifndef RTX_RBUF_GLOBAL_N
#define RTX_RBUF_GLOBAL_N 160      // C4: 294.5 / 285.6 / 283.7 ms per frame at 40 / 80 / 160 (r11y; r11ab: 285.4 / 283.2 at 80 / 160; 77 MB)
#endif

namespace rtx {

// Everything rtx_scene_upload sends: the arrays, and `dev` with SceneDev's scalars (its pointers stay
// null here).  The builder refers to the sphere arrays, so a HostScene is neither copied nor moved.
struct HostScene {
  SceneDev dev{};
  std::vector<Run> runs;
  std::vector<Material> mat;
  std::vector<Sphere64> sph64;
  std::vector<float> sph32;                    // pack_objects appends 4 padding records: group loads stay in bounds
  std::vector<int32_t> sph_obj;
  std::vector<double> planes, boxes;
  std::vector<BSph> bs;                        // the builder's working order of the spheres
  std::unique_ptr<Bvh4Builder> bb;             // nodes, slot32, slot64, slot_obj (build_hierarchy)
  QuantLeaves ql;
  std::vector<LightDev> lights;
  std::vector<TexDev> tex;
  std::vector<uint8_t> texels;
  std::vector<double> lpos, lrad, lfloor;      // per light: position (3), radius, raise floor (raise_floors)
  LightBuffer lb;
  RaiseBuffer rb;
  std::vector<uint16_t> gates;                 // per light dev.rgate_stride words (pack_gates)
  HostScene() = default;
  HostScene(const HostScene&) = delete;
  HostScene& operator=(const HostScene&) = delete;
  const double (*light_pos() const)[3] { return reinterpret_cast<const double(*)[3]>(lpos.data()); }
};

inline rtx_status fail(std::string& err, rtx_status s, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  err = buf;
  return s;
}
inline void put3(std::vector<double>& g, V3 v) { g.insert(g.end(), {v.x, v.y, v.z}); }
inline void set3(double* d, V3 v) { d[0] = v.x, d[1] = v.y, d[2] = v.z; }
// Plane record (plane.rb:21-23 reinit + get_uv's re-normalizations :82-83).
inline void put_plane(std::vector<double>& g, V3 P, V3 F, V3 U, double uu, double vu, uint32_t& err) {
  V3 left = vnorm(vcross(F, U), err);
  put3(g, P);
  put3(g, F);
  put3(g, vnorm(left, err));
  put3(g, vnorm(U, err));
  g.push_back(uu);
  g.push_back(vu);
}

// One sphere's records: binary64, the float32 pre-test record {cx, cy, cz, R^2},
// its object index, and the scene's scale = max(|C|_1 + R) (exact culls).
inline void pack_sphere(HostScene& H, int obj, const double c[3], double r) {
  H.sph_obj.push_back(obj);
  H.sph64.push_back(Sphere64{{c[0], c[1], c[2]}, r});
  H.sph32.insert(H.sph32.end(), {(float)c[0], (float)c[1], (float)c[2], (float)(r * r)});
  const double sc = fabs(c[0]) + fabs(c[1]) + fabs(c[2]) + fabs(r);
  const float scf = (float)(sc * (1.0 + 1e-6));
  if (scf > H.dev.sph_scale) H.dev.sph_scale = scf;
}

// Materials, runs and the sphere / plane / box records.
inline rtx_status pack_objects(const rtx_scene_desc* sd, HostScene& H, std::string& msg) {
  uint32_t err = 0;
  H.mat.resize(sd->n_objects);
  for (int i = 0; i < sd->n_objects; i++) {
    const rtx_object_desc& o = sd->objects[i];
    Material& m = H.mat[i];
    memset(&m, 0, sizeof m);
    set3(m.diffuse, v3p(o.diffuse_rate));
    set3(m.ambient, v3p(o.ambient));
    set3(m.refl_att, v3p(o.reflective_attenuation));
    set3(m.refr_att, v3p(o.refractive_attenuation));
    m.rr = o.refractive_rate;
    m.has_rr = o.has_refractive_rate != 0;
    m.tex = o.texture_id;
    m.hs = o.texture_horizontal_scale;
    m.vs = o.texture_vertical_scale;
    m.type = o.type;
    if (o.texture_id >= sd->n_textures) return fail(msg, RTX_EINVAL, "object %d: bad texture id", i);
    if (o.type != RTX_SPHERE && o.type != RTX_PLANE && o.type != RTX_BOX)
      return fail(msg, RTX_EINVAL, "object %d: unknown type %d", i, o.type);
    if (H.runs.empty() || H.runs.back().type != o.type) {
      const int rec0 = o.type == RTX_SPHERE ? (int)H.sph64.size()
                     : o.type == RTX_PLANE ? (int)(H.planes.size() / PLANE_GEO) : (int)(H.boxes.size() / BOX_GEO);
      H.runs.push_back(Run{o.type, i, 0, rec0});
    }
    H.runs.back().count++;
    if (o.type == RTX_SPHERE) {
      if (!o.has_refractive_rate) return fail(msg, RTX_EINVAL, "object %d: sphere needs refractive_rate", i);
      m.rec = (int)H.sph64.size();
      pack_sphere(H, i, o.center, o.radius);
      m.u_off = o.texture_u_offset;
      m.v_off = o.texture_v_offset;
      if (o.texture_id >= 0) {                     // sphere.rb:18, 113-115
        const V3 north = v3p(o.north_pole_vec), gw = v3p(o.greenwich_vec);
        set3(m.gw_n, vnorm(gw, err));
        set3(m.east_n, vnorm(vcross(north, gw), err));
        set3(m.north_n, vnorm(north, err));
      }
    } else if (o.type == RTX_PLANE) {
      m.rec = (int)(H.planes.size() / PLANE_GEO);
      put_plane(H.planes, v3p(o.point), v3p(o.front), v3p(o.up), o.u_unit, o.v_unit, err);
    } else {                                         // box.rb:15-73
      m.rec = (int)(H.boxes.size() / BOX_GEO);
      m.tex = -1;                                    // loaded, never used for shading
      const V3 P = v3p(o.point), F = v3p(o.front), U = v3p(o.up);
      const double wf = o.width_front, wu = o.width_up, wl = o.width_left;
      const V3 left = vnorm(vcross(F, U), err);
      put_plane(H.boxes, vadd(P, vsc(vsc(U, wu), 0.5)), U, left, wf, wl, err);
      put_plane(H.boxes, vsub(P, vsc(vsc(U, wu), 0.5)), vneg(U), left, wf, wl, err);
      put_plane(H.boxes, vadd(P, vsc(vsc(F, wf), 0.5)), F, U, wl, wu, err);
      put_plane(H.boxes, vsub(P, vsc(vsc(F, wf), 0.5)), vneg(F), U, wl, wu, err);
      put_plane(H.boxes, vadd(P, vsc(vsc(left, wl), 0.5)), left, U, wf, wu, err);
      put_plane(H.boxes, vsub(P, vsc(vsc(left, wl), 0.5)), vneg(left), U, wf, wu, err);
    }
  }
  if (err) return fail(msg, RTX_EZERO_VEC, "zero vector detected while building the scene");
  if (!std::isfinite(H.dev.sph_scale)) return fail(msg, RTX_EINVAL, "non-finite sphere coordinates");
  for (int k = 0; k < 16; k++) H.sph32.push_back(0.0f);
  H.dev.n_obj = sd->n_objects;
  H.dev.n_sphere = (int)H.sph64.size();
  H.dev.n_plane = (int)(H.planes.size() / PLANE_GEO);
  H.dev.n_box = (int)(H.boxes.size() / BOX_GEO);
  H.dev.n_runs = (int)H.runs.size();
  return RTX_OK;
}

// The bounding-ball hierarchy over H's spheres.  With `lds_fallback`: SAH splits unless their tree
// would not fit the LDS of a hierarchy workgroup while the median tree does (C4: the SAH tree spills to
// global memory and renders 10 % slower; C2: SAH 1.3 % faster).
inline void build_hierarchy(HostScene& H, bool sah, bool lds_fallback = true) {
  auto grow = [&H](bool with_sah, int32_t& root) {
    H.bs.resize(H.sph64.size());
    for (size_t k = 0; k < H.sph64.size(); k++) {
      for (int a = 0; a < 3; a++) H.bs[k].c[a] = H.sph64[k].c[a];
      H.bs[k].r = H.sph64[k].r;
      H.bs[k].rec = (int)k;
    }
    auto b = std::make_unique<Bvh4Builder>(Bvh4Builder{H.bs, H.sph64, H.sph32, H.sph_obj});
    b->sah = with_sah;
    root = H.bs.empty() ? BVH_NONE : b->build(0, (int)H.bs.size(), 0);
    return b;
  };
  auto fits = [](const Bvh4Builder& b) {
    return bvh_lds_bytes((int)b.nodes.size(), (int)b.slot_obj.size(), b.stack + 1) <= bvh_lds_budget();
  };
  int32_t root;
  H.bb = grow(sah, root);
  if (sah && lds_fallback && !H.bs.empty() && !fits(*H.bb)) {
    int32_t r;
    auto med = grow(false, r);                 // (reorders H.bs; a built tree no longer reads it)
    if (fits(*med)) {
      H.bb = std::move(med);
      root = r;
    }
  }
  H.dev.n_nodes = (int)H.bb->nodes.size();
  H.dev.n_slots = (int)H.bb->slot_obj.size();
  H.dev.bvh_root = root;
  H.dev.bvh_stack = H.bb->stack + 1;
}

// The 16-bit leaf records of the hierarchy and their decoding scalars.
inline void pack_quantized_leaves(HostScene& H) {
  SceneDev& S = H.dev;
  H.ql = quantize_leaves(*H.bb, S.sph_scale);
  const QuantLeaves& ql = H.ql;
  for (int a = 0; a < 3; a++) S.q_org[a] = ql.org[a], S.q_step[a] = ql.step[a];
  S.q_rstep = ql.rstep;
  S.q_ok = ql.ok && S.n_nodes <= 32767 && (int64_t)S.n_slots <= 32767;   // references fit int16 stack entries
  // a decoded center lies within max_err of the true one; a decoded radius within max_err + 2 rstep of R
  // (ceil to the step, at most one more step: quantize_leaves)
  S.q_err = (float)((ql.max_err + 2.0 * (double)ql.rstep) * 1.01 + 1e-9 * ql.max_r);
}

// The lights, with the squared-cosine bands of the highlight test.
inline void pack_lights(const rtx_scene_desc* sd, HostScene& H) {
  H.lights.resize(sd->n_lights);
  H.lpos.assign(3 * (size_t)std::max(1, sd->n_lights), 0.0);
  H.lrad.assign(std::max(1, sd->n_lights), 0.0);
  for (int i = 0; i < sd->n_lights; i++) {
    const rtx_light_desc& l = sd->lights[i];
    LightDev& d = H.lights[i];
    memset(&d, 0, sizeof d);
    set3(d.pos, v3p(l.position));
    set3(d.color, v3p(l.color));
    d.radius = l.radius;
    d.hl_rate = l.high_light_rate;
    d.hl_angle_rad = l.high_light_angle / 180.0 * 3.141592653589793;   // world.rb:91
    const double th = d.hl_angle_rad;
    if (!(th > 0)) {
      d.hl_mode = 2;                                 // acos(c) >= 0 can never be < th
    } else if (th < 1e-6 || th > 1.5) {
      d.hl_mode = 1;
    } else {
      const double ct = cos(th), lo = ct - 1e-7, hi = ct + 1e-7;
      d.hl_mode = (hi >= 1.0 || lo <= 0.0) ? 1 : 0;
      d.cos_lo2 = lo * lo;
      d.cos_hi2 = hi * hi;
    }
    for (int a = 0; a < 3; a++) H.lpos[3 * i + a] = d.pos[a];
    H.lrad[i] = d.radius;
  }
  H.dev.n_light = sd->n_lights;
}

inline rtx_status pack_textures(const rtx_scene_desc* sd, HostScene& H, std::string& msg) {
  H.tex.resize(sd->n_textures);
  for (int i = 0; i < sd->n_textures; i++) {
    const rtx_texture_desc& t = sd->textures[i];
    if (t.width <= 0 || t.height <= 0 || !t.rgb) return fail(msg, RTX_EINVAL, "texture %d: empty", i);
    H.tex[i].w = t.width;
    H.tex[i].h = t.height;
    H.tex[i].off = (int64_t)H.texels.size();
    H.texels.insert(H.texels.end(), t.rgb, t.rgb + (size_t)t.width * t.height * 3);
  }
  return RTX_OK;
}

// Each light's raise-buffer floor: 0.99 of the distance to the nearest object
// surface (targets of World#local_lights lie on surfaces; nearer ones walk the
// hierarchy).
inline std::vector<double> raise_floors(const rtx_scene_desc* sd) {
  std::vector<double> lfloor(std::max(1, sd->n_lights), 0.0);
  for (int li = 0; li < sd->n_lights; li++) {
    const double* L = sd->lights[li].position;
    double fl = HUGE_VAL;
    for (int k = 0; k < sd->n_objects; k++) {
      const rtx_object_desc& o = sd->objects[k];
      auto dist = [&](const double* p) {
        return std::sqrt((L[0] - p[0]) * (L[0] - p[0]) + (L[1] - p[1]) * (L[1] - p[1]) + (L[2] - p[2]) * (L[2] - p[2]));
      };
      auto norm = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
      if (o.type == RTX_SPHERE) {
        fl = std::min(fl, dist(o.center) - std::fabs(o.radius));
      } else if (o.type == RTX_PLANE) {
        const double fn = norm(o.front);
        fl = std::min(fl, std::fabs((L[0] - o.point[0]) * o.front[0] + (L[1] - o.point[1]) * o.front[1] +
                                    (L[2] - o.point[2]) * o.front[2]) / fn);
      } else {                                    // a box: within this ball of its point (box.rb:15-73)
        const double rb = 0.5 * (std::fabs(o.width_front) * (1.0 + norm(o.front)) +
                                 std::fabs(o.width_up) * (1.0 + norm(o.up)) + 2.0 * std::fabs(o.width_left));
        fl = std::min(fl, dist(o.point) - rb);
      }
    }
    lfloor[li] = std::isfinite(fl) ? std::max(0.0, 0.99 * fl) : 0.0;
  }
  return lfloor;
}

inline bool small_scene(const HostScene& H) { return H.sph64.size() <= 512; }

// The light buffer, at the finest resolution that fits.  Small
// scenes: a table for LDS (<= 16 KB); larger ones: a finer one read from global
// memory (<= 512 KB, L2-resident).
inline void choose_light_buffer(HostScene& H) {
  const bool small = small_scene(H);
  const int nl = H.dev.n_light;
  H.lb = LightBuffer{};
  if (nl > 0 && !H.sph64.empty())
    for (int n : small ? std::vector<int>{24, 16, 12, 8} : std::vector<int>{RTX_LBUF_GLOBAL_N, 128, 96, 64, 48, 32, 24}) {
      H.lb = build_light_buffer(*H.bb, H.dev.bvh_root, H.light_pos(), nl, n,
                                small ? LBUF_MAX_WORDS : LBUF_MAX_WORDS_GLOBAL, H.lrad.data());
      if (H.lb.n) break;
    }
  H.dev.lbuf_n = H.lb.n;
  H.dev.lbuf_stride = H.lb.stride;
}

// The raise buffer (exact_raises): its cells nest in the light buffer's (small scenes:
// 12 per face side for C2's 24, gates staged in LDS; larger: 160, as C4's light buffer), read from
// global memory.  The finest nesting resolution up to 12 / 160 cells per face side whose lists fit at
// the lights' own floors (H.lfloor); only if none does, a coarse one with the floors raised until it
// fits.
inline void choose_raise_buffer(HostScene& H) {
  const bool small = small_scene(H);
  const int nl = H.dev.n_light;
  H.rb = RaiseBuffer{};
  const int want = small ? 12 : RTX_RBUF_GLOBAL_N;
  const size_t rb_max = small ? RBUF_MAX_WORDS : RBUF_MAX_WORDS_GLOBAL;
  int coarse = 0;
  for (int nc = std::min(want, H.lb.n); nc >= 1 && !H.rb.n; nc--) {
    if (H.lb.n % nc) continue;
    coarse = nc;
    if (nc < 4) break;
    H.rb = build_raise_buffer(*H.bb, H.dev.bvh_root, H.light_pos(), H.lrad.data(), H.lfloor.data(), nl, nc, rb_max,
                              !small, 0);
  }
  if (!H.rb.n && coarse)
    H.rb = build_raise_buffer(*H.bb, H.dev.bvh_root, H.light_pos(), H.lrad.data(), H.lfloor.data(), nl, coarse, rb_max,
                              !small);
  if (!H.rb.n) return;
  H.dev.rbuf_n = H.rb.n;
  H.dev.rbuf_stride = H.rb.stride;
  H.dev.rbuf_inv_m = (float)H.rb.n / (float)H.lb.n;   // (exact enough: (i + 0.5) m' stays 0.5 / m from an integer)
  H.dev.rbuf_sphere = small ? 0 : 1;                  // larger scenes: per-sphere entries (fewer band tests per walk)
}

// The gate blocks of the raise buffer, per light: floor^2 (rounded up) and log2 floor^2 (float bits, 2
// words each), 4 words of padding, a gate word per cell from word 8 (rtx_device.h raise_qa).  The
// lights carry the two floats too.
inline void pack_gates(HostScene& H) {
  H.gates.clear();
  if (!H.rb.n) return;
  const int nl = H.dev.n_light;
  const std::vector<uint16_t> g = raise_gates(H.rb, nl);
  const int cells = 6 * H.rb.n * H.rb.n, gs = (8 + cells + 7) & ~7;
  H.gates.assign((size_t)gs * nl, 0);
  for (int li = 0; li < nl; li++) {
    const float hw[2] = {raise_floor2(H.rb, li), raise_lf2(H.rb, li)};
    memcpy(&H.gates[(size_t)gs * li], hw, 8);
    std::copy(g.begin() + (size_t)cells * li, g.begin() + (size_t)cells * (li + 1), H.gates.begin() + (size_t)gs * li + 8);
    H.lights[li].raise_f2 = hw[0];              // (raise_qa reads them with the light's data)
    H.lights[li].raise_lf2 = hw[1];
  }
  H.dev.rgate_stride = gs;
}

// The spheres' box, float32, rounded outwards.
inline void sphere_box(HostScene& H) {
  SceneDev& S = H.dev;
  double mn[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, mx[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
  for (const Sphere64& sp : H.sph64)
    for (int a = 0; a < 3; a++) {
      mn[a] = std::min(mn[a], sp.c[a] - fabs(sp.r));
      mx[a] = std::max(mx[a], sp.c[a] + fabs(sp.r));
    }
  for (int a = 0; a < 3; a++) {
    if (!(mn[a] <= mx[a])) {                       // no spheres: an empty box far away
      S.root_c[a] = 3e38f;
      S.root_h[a] = 0.0f;
      continue;
    }
    const float cf = (float)(0.5 * (mn[a] + mx[a]));
    const double h = std::max(mx[a] - (double)cf, (double)cf - mn[a]);
    S.root_c[a] = cf;
    S.root_h[a] = f32_up(h * (1.0 + 1e-9) + 1e-30);
  }
}

// The whole build, in rtx_scene_upload's order.  `H` must be fresh.
inline rtx_status build_host_scene(const rtx_scene_desc* sd, bool sah, HostScene& H, std::string& msg) {
  if (!sd) return fail(msg, RTX_EINVAL, "null argument");
  if (sd->n_objects < 0 || sd->n_lights < 0 || sd->n_textures < 0) return fail(msg, RTX_EINVAL, "negative counts");
  if (sd->n_lights > 32) return fail(msg, RTX_EINVAL, "at most 32 lights are supported");
  if ((sd->n_objects && !sd->objects) || (sd->n_lights && !sd->lights) || (sd->n_textures && !sd->textures))
    return fail(msg, RTX_EINVAL, "null array with nonzero count");
  if (rtx_status st = pack_objects(sd, H, msg)) return st;
  build_hierarchy(H, sah);
  pack_quantized_leaves(H);
  pack_lights(sd, H);
  if (rtx_status st = pack_textures(sd, H, msg)) return st;
  choose_light_buffer(H);
  if (H.lb.n) {
    H.lfloor = raise_floors(sd);
    choose_raise_buffer(H);
    pack_gates(H);
  }
  sphere_box(H);
  H.dev.max_distance = sd->max_distance;
  H.dev.sse = sd->soft_shadow_exponent;
  H.dev.sse_is_two = sd->soft_shadow_exponent == 2.0;     // glibc pow(x, 2.0) == x*x
  return RTX_OK;
}

}  // namespace rtx
