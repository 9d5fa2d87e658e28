// rtx_aov.hip — first-hit feature buffers (DESIGN.md "Feature buffers"): for
// one camera sample's primary ray of every pixel of a rectangle,
//
//   Camera#lens_func(x, y, sample)   (src/camera.rb:129-151)
//   World#intersect(ray)             (src/world.rb:37-59)
//
// and, for the object hit, what intersect / intersect_parameters / get_uv /
// Texture#color give without any shading (sphere.rb:60-120, plane.rb:38-85,
// box.rb:79-105, texture.rb:23-28):
//
//   ids[3]   = {object (YAML index), direction (0 :in, 1 :out), data (box face, else -1)}
//   geom[10] = {depth, intersection xyz, n.normalize xyz, albedo rgb}
//
// A miss is {-1, -1, -1} and {max_distance, 0 ...}.  Highlights are not
// consulted and nothing is raised: the walk's error word is dropped.
//
// k_intersect answers the same question for explicit rays (rtx_intersect,
// DESIGN.md "Batched World queries"): one ray per lane, consecutive rays in
// consecutive lanes, 13-value records whose last three are the `delta`
// World#intersect returns.
//
// k_first_hit: one pixel per lane, one wave per 8x8 pixel tile (lane l = pixel (l & 7,
// l >> 3) of the tile), four tiles side by side per 256-thread workgroup: the
// 64 rays of a wave start together, and the 8 lanes of a tile row (the 32 of a
// workgroup row) store contiguous records.  Every value is computed by the
// device functions of the colour path (rtx_device.h), in binary64 with the
// reference's operation order (-ffp-contract=off).
#include "rtx_device.h"

namespace rtx {

constexpr int FH_BS = 256;

// Record idx of World#intersect(ray).  SPH: SPH_LIN_SCALAR (ordered linear
// walk), SPH_BVH_LDS (hierarchy nodes and leaf records staged in LDS) or
// SPH_BVH_GLOBAL (read from global memory); the hierarchy walks keep their
// per-lane traversal stacks in LDS (p.lds_stack).  NG: doubles per geom record,
// 10 (k_first_hit) or 13 (k_intersect: delta appended).
template <int SPH, int NG>
__device__ __forceinline__ void first_hit_ray(const KParams& p, char* lds, const Ray& ray, size_t idx,
                                              int32_t* __restrict__ ids, double* __restrict__ geom) {
  const SceneDev& S = p.scene;                  // kernel argument: scalar loads

  double best = S.max_distance, total = 0.0;
  int besti = -1;
  bool hin = true;
  uint32_t err = 0;                             // dropped: this pass raises nothing
  V3 hit = v3(0.0, 0.0, 0.0);
  if (SPH == SPH_LIN_SCALAR) {
    query<false>(S, cptr(S.sph32), true, ray.o, ray.d, hit, 0.0, best, besti, hit, hin, total, err, nullptr);
  } else {
    int* stk = reinterpret_cast<int*>(lds + p.lds_stack) + threadIdx.x;
    int q_ref = BVH_NONE, q_sp = 0, q_ncov = 0;
    bool q_ovf = false;
    if (SPH == SPH_BVH_LDS)
      query_bvh<FH_BS, false>(S, reinterpret_cast<const Bvh4Node*>(lds),
                              reinterpret_cast<const float4*>(lds + p.lds_leaf), S.bvh_sph64, S.bvh_obj, stk,
                              (int*)nullptr, (double*)nullptr, true, ray.o, ray.d, hit, 0.0, best, besti, hit, hin,
                              total, err, q_ref, q_sp, q_ncov, q_ovf, false, 0);
    else
      query_bvh<FH_BS, false>(S, S.bvh, reinterpret_cast<const float4*>(S.bvh_sph32), S.bvh_sph64, S.bvh_obj, stk,
                              (int*)nullptr, (double*)nullptr, true, ray.o, ray.d, hit, 0.0, best, besti, hit, hin,
                              total, err, q_ref, q_sp, q_ncov, q_ovf, false, 0);
  }

  int dir = -1, data = -1;
  V3 nn = v3(0.0, 0.0, 0.0), alb = nn, delta = nn;
  if (besti >= 0) {
    const Material& m = S.mat[besti];
    V3 n;
    hit_info(S, besti, ray, hit, delta, n, hin);          // (boxes: re-evaluates the hit)
    const double* plane = nullptr;                        // the plane, or the box face, hit
    if (m.type == OBJ_SPHERE) {
      dir = hin ? 0 : 1;                                  // from_inner -> :out (sphere.rb:74-76)
    } else {
      plane = S.planes + (size_t)m.rec * PLANE_GEO;
      if (m.type == OBJ_BOX) {                            // the face Box#intersect returns as data (box.rb:79-97)
        V3 h;
        int face = 0;
        box_hit(S.boxes + (size_t)m.rec * BOX_GEO, ray.o, ray.d, h, face);
        data = face;
        plane = S.boxes + (size_t)m.rec * BOX_GEO + face * PLANE_GEO;
      }
      dir = vdot(v3(plane[3], plane[4], plane[5]), ray.d) < 0 ? 0 : 1;   // plane.rb:45-49
    }
    const double nr = vr(n);                              // n.normalize; a zero n gives zeros
    if (nr != 0) nn = vdiv(n, nr);
    alb = v3p(m.diffuse);
    if (m.tex >= 0 && m.type != OBJ_BOX) {                // diffuse_rate * texture.color(*get_uv(intersection))
      uint32_t terr = 0;
      V3 tc;
      double u, v;
      if (m.type == OBJ_SPHERE) {                         // (a negative sqrt argument: a NaN uv, zeros below)
        double mm2;
        sphere_uv(S, m, hit, u, v, mm2);
        tc = texcolor(S, m.tex, m.hs, m.vs, m.u_off, m.v_off, u, v, terr);
      } else {                                            // Plane#get_uv (plane.rb:81-85)
        plane_uv(plane, hit, u, v);
        tc = texcolor(S, m.tex, m.hs, m.vs, 0.0, 0.0, u, v, terr);
      }
      alb = terr ? v3(0.0, 0.0, 0.0) : vmul(alb, tc);     // a non-finite uv gives zeros
    }
  }                                                       // (a miss: best is still max_distance, hit zeros)

  if (ids) {
    int32_t* o = ids + idx * 3;
    o[0] = besti;
    o[1] = dir;
    o[2] = data;
  }
  if (geom) {
    double* g = geom + idx * NG;                          // 80-byte (104-byte) records
    // (13 doubles: in a 16-byte aligned buffer the odd records start 8 bytes off.  Those store the depth
    // alone and pairs after it, the even ones pairs and delta z alone; the scalar stores serve a buffer
    // that is only 8-byte aligned.)
    const bool al = (reinterpret_cast<uintptr_t>(geom) & 15) == 0;
    if (al && (NG == 10 || !(idx & 1))) {
      double2* g2 = reinterpret_cast<double2*>(g);
      g2[0] = make_double2(best, hit.x);
      g2[1] = make_double2(hit.y, hit.z);
      g2[2] = make_double2(nn.x, nn.y);
      g2[3] = make_double2(nn.z, alb.x);
      g2[4] = make_double2(alb.y, alb.z);
      if (NG == 13) {
        g2[5] = make_double2(delta.x, delta.y);
        g[12] = delta.z;
      }
    } else if (NG == 13 && al) {
      double2* g2 = reinterpret_cast<double2*>(g + 1);
      g[0] = best;
      g2[0] = make_double2(hit.x, hit.y);
      g2[1] = make_double2(hit.z, nn.x);
      g2[2] = make_double2(nn.y, nn.z);
      g2[3] = make_double2(alb.x, alb.y);
      g2[4] = make_double2(alb.z, delta.x);
      g2[5] = make_double2(delta.y, delta.z);
    } else {
      g[0] = best;
      g[1] = hit.x, g[2] = hit.y, g[3] = hit.z;
      g[4] = nn.x, g[5] = nn.y, g[6] = nn.z;
      g[7] = alb.x, g[8] = alb.y, g[9] = alb.z;
      if (NG == 13) g[10] = delta.x, g[11] = delta.y, g[12] = delta.z;
    }
  }
}

// The lens wrapper: the record of pixel (px_, row) of the region, its ray Camera#lens_func's.
template <int SPH>
__device__ __forceinline__ void first_hit_pixel(const KParams& p, char* lds, int sample, int px_, int row,
                                                int32_t* __restrict__ ids, double* __restrict__ geom) {
  const CameraDev& cam = *p.cam;
  const int x = p.x0 + px_, y = p.y0 + row;
  const Ray ray = lens_ray(cam, lens_target(cam, x, y), x, y, sample, p.seed);
  first_hit_ray<SPH, 10>(p, lds, ray, (size_t)row * (size_t)p.nx + (size_t)px_, ids, geom);
}

// SPH_BVH_LDS: the workgroup's copy of the hierarchy's nodes and leaf records (the only barrier).
template <int SPH>
__device__ __forceinline__ void fh_stage(const KParams& p, float4* lds4) {
  const SceneDev& S = p.scene;
  if (SPH == SPH_BVH_LDS) {
    const int nn = S.n_nodes * (int)(sizeof(Bvh4Node) / 16);
    for (int i = threadIdx.x; i < nn; i += FH_BS) lds4[i] = reinterpret_cast<const float4*>(S.bvh)[i];
    float4* leaf = reinterpret_cast<float4*>(reinterpret_cast<char*>(lds4) + p.lds_leaf);
    for (int i = threadIdx.x; i < S.n_slots; i += FH_BS) leaf[i] = reinterpret_cast<const float4*>(S.bvh_sph32)[i];
    __syncthreads();
  }
}

// One workgroup per strip of FH_BS / 64 tiles side by side (32 x 8 pixels), one
// tile per wave.  (A persistent grid that stages C4's hierarchy once per
// resident workgroup and takes strips grid-stride measured 1.56 ms per frame
// against 0.8 ms for this grid reading it from global memory)
template <int SPH>
__global__ __launch_bounds__(FH_BS) void k_first_hit(KParams p, int sample, int32_t* __restrict__ ids,
                                                      double* __restrict__ geom) {
  extern __shared__ float4 lds_fh[];
  char* lds = reinterpret_cast<char*>(lds_fh);
  fh_stage<SPH>(p, lds_fh);
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int px_ = ((int)blockIdx.x * (FH_BS / 64) + wave) * 8 + (lane & 7);
  const int row = (int)blockIdx.y * 8 + (lane >> 3);
  if (px_ >= p.nx || row >= p.nrows) return;
  first_hit_pixel<SPH>(p, lds, sample, px_, row, ids, geom);
}

// World#intersect for the explicit rays p.rays[0 .. p.nrays) (6 doubles each: front, position, as
// rtx_trace): ray i in lane i mod 64 of wave i / 64.  A lane past the batch leaves before the walk
// (the hierarchy walk ballots over the lanes that entered it).
template <int SPH>
__global__ __launch_bounds__(FH_BS) void k_intersect(KParams p, int32_t* __restrict__ ids, double* __restrict__ geom) {
  extern __shared__ float4 lds_fh[];
  fh_stage<SPH>(p, lds_fh);
  const size_t i = (size_t)blockIdx.x * FH_BS + threadIdx.x;
  if (i >= (size_t)p.nrays) return;
  Ray ray;
  ray.d = v3p(p.rays + 6 * i);
  ray.o = v3p(p.rays + 6 * i + 3);
  first_hit_ray<SPH, 13>(p, reinterpret_cast<char*>(lds_fh), ray, i, ids, geom);
}

template <int SPH>
static hipError_t launch_fh(const KParams& p, size_t lds, int32_t sample, int32_t* d_ids, double* d_geom,
                            hipStream_t s) {
  const int tiles_x = (p.nx + 7) / 8, tiles_y = (p.nrows + 7) / 8;
  if (tiles_y > 65535) return hipErrorInvalidValue;               // grid rows
  const dim3 grid((unsigned)((tiles_x + FH_BS / 64 - 1) / (FH_BS / 64)), (unsigned)tiles_y);
  hipLaunchKernelGGL(k_first_hit<SPH>, grid, dim3(FH_BS), lds, s, p, (int)sample, d_ids, d_geom);
  return hipGetLastError();
}

// Workgroups per CU the kernel's registers allow (4 waves per SIMD): the
// hierarchy is staged only while its LDS image leaves that occupancy.
constexpr int FH_WGS_PER_CU = 4;

// mode: the context's SphMode (rtx_capi.cpp sph_mode).  A linear mode walks the
// ordered scan; every hierarchy mode walks the four-wide hierarchy in EXTEND
// mode.  Its nodes and leaf records are staged in LDS when they fit: the
// hierarchy workgroup's layout by resolve_mode (bvh_lds_bytes), and this
// kernel's own image (records + traversal stacks) FH_WGS_PER_CU times per CU.
// Otherwise they are read from global memory (C4: 101 KB of records would leave
// one workgroup per CU, each staging them for 256 pixels: 2.15 ms per 3840x2160
// frame against 0.78 ms from global memory).
// Returns the walk (SPH_LIN_SCALAR, SPH_BVH_LDS or SPH_BVH_GLOBAL), fills p's LDS layout and `lds`, its bytes.
static hipError_t fh_layout(KParams& p, int mode, int& sph, size_t& lds) {
  const SceneDev& S = p.scene;
  sph = SPH_LIN_SCALAR;
  lds = 0;
  if (!sph_is_bvh(mode) || S.bvh_root == BVH_NONE) return hipSuccess;
  const size_t stacks = (size_t)S.bvh_stack * FH_BS * 4;   // per-lane traversal stacks (no cover lists: EXTEND only)
  const size_t image = (((size_t)S.n_nodes * sizeof(Bvh4Node) + (size_t)S.n_slots * 16 + 15) & ~(size_t)15) + stacks;
  const bool staged = mode != SPH_BVH_GLOBAL && resolve_mode(S, SPH_BVH_LDS) == SPH_BVH_LDS &&
                      image <= LDS_TOTAL_BYTES / FH_WGS_PER_CU;
  size_t off = 0;
  if (staged) {
    off = (size_t)S.n_nodes * sizeof(Bvh4Node);
    p.lds_leaf = (int32_t)off;
    off += (size_t)S.n_slots * 16;
    off = (off + 15) & ~(size_t)15;
  }
  p.lds_stack = (int32_t)off;
  off += stacks;
  if (off > 64 * 1024) return hipErrorInvalidValue;   // (a traversal stack deeper than 64 entries: no hierarchy built here is)
  sph = staged ? SPH_BVH_LDS : SPH_BVH_GLOBAL;
  lds = off;
  return hipSuccess;
}

hipError_t launch_first_hit(KParams p, int mode, int32_t sample, int32_t* d_ids, double* d_geom, hipStream_t s) {
  if (p.nx <= 0 || p.nrows <= 0) return hipSuccess;
  int sph;
  size_t lds;
  const hipError_t e = fh_layout(p, mode, sph, lds);
  if (e != hipSuccess) return e;
  return sph == SPH_LIN_SCALAR ? launch_fh<SPH_LIN_SCALAR>(p, lds, sample, d_ids, d_geom, s)
         : sph == SPH_BVH_LDS  ? launch_fh<SPH_BVH_LDS>(p, lds, sample, d_ids, d_geom, s)
                               : launch_fh<SPH_BVH_GLOBAL>(p, lds, sample, d_ids, d_geom, s);
}

// The same walks and the same staging rule for p.nrays explicit rays (p.rays, device memory).
hipError_t launch_intersect(KParams p, int mode, int32_t* d_ids, double* d_geom, hipStream_t s) {
  if (p.nrays <= 0) return hipSuccess;
  int sph;
  size_t lds;
  const hipError_t e = fh_layout(p, mode, sph, lds);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)(((size_t)p.nrays + FH_BS - 1) / FH_BS));
  if (sph == SPH_LIN_SCALAR) hipLaunchKernelGGL(k_intersect<SPH_LIN_SCALAR>, grid, dim3(FH_BS), lds, s, p, d_ids, d_geom);
  else if (sph == SPH_BVH_LDS) hipLaunchKernelGGL(k_intersect<SPH_BVH_LDS>, grid, dim3(FH_BS), lds, s, p, d_ids, d_geom);
  else hipLaunchKernelGGL(k_intersect<SPH_BVH_GLOBAL>, grid, dim3(FH_BS), lds, s, p, d_ids, d_geom);
  return hipGetLastError();
}

}  // namespace rtx
