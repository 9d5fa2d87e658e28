// rtx_pixels.hip — Camera#render_at for a list of pixels (rtx_render_pixels,
// DESIGN.md §3.23): what surrounds the two traces of a chunk of the list.
//
//   k_pixel_rays        lens_func(x, y, j), j < pre, for every pixel: rays and RNG keys
//   (the trace)         launch_trace_levels: a colour and a status per sample
//   k_pixel_reduce      render_at's pixel stage (camera.rb:70-99): mean, variance, the test
//                       against variant_threshold; the pixels that take extra samples are
//                       listed, the count of the list stays on the device
//   k_pixel_extra_rays  lens_func(x, y, j), j = pre .. max - 1, for the listed pixels
//   (the trace)         the same, its live ray count read from device memory
//   k_pixel_finish      (mean * pre + the extra samples) / max for the listed pixels
//
// The rays are the render's own (lens_target / lens_ray of rtx_device.h, as
// k_lens_rays and level 0 of a render), the arithmetic is lv_tile_pixels' and
// k_tree_finalize_extra's operation for operation (rtx_levels.hip), and a
// sample's colour does not depend on the engine or batch that traced it, so a
// pixel's colour has the bits rtx_render writes for it.  Nothing goes to the
// raise record: a raising pixel's status is in info, its colour is NaN.
#include <hip/hip_runtime.h>

#include "rtx_device.h"

namespace rtx {

constexpr int PX_BS = 256;

// (the chunk's buffers come 256-byte aligned from one allocation: 48-byte ray records are 16-byte aligned)
__device__ __forceinline__ void px_store_ray(double* g, const Ray& r, int32_t* k, int x, int y, int j) {
  double2* g2 = reinterpret_cast<double2*>(g);
  g2[0] = make_double2(r.d.x, r.d.y);
  g2[1] = make_double2(r.d.z, r.o.x);
  g2[2] = make_double2(r.o.y, r.o.z);
  k[0] = x;
  k[1] = y;
  k[2] = j;
}

// The caller's output buffers may be only 8-byte aligned: scalar stores.
__device__ __forceinline__ void px_store3(double* o, V3 a) {
  o[0] = a.x;
  o[1] = a.y;
  o[2] = a.z;
}

__global__ __launch_bounds__(PX_BS) void k_pixel_rays(const CameraDev* __restrict__ camp, uint64_t seed,
                                                       const int32_t* __restrict__ xy, int npx, int pre,
                                                       double* __restrict__ rays, int32_t* __restrict__ keys,
                                                       int32_t* __restrict__ count) {
  const size_t t = (size_t)blockIdx.x * PX_BS + threadIdx.x;
  if (t == 0) count[0] = count[1] = 0;          // (the chunk's list is empty until k_pixel_reduce)
  if (t >= (size_t)npx * (size_t)pre) return;
  const CameraDev& cam = *camp;
  const size_t i = t / (size_t)pre;
  const int j = (int)(t - i * (size_t)pre);
  const int x = xy[2 * i], y = xy[2 * i + 1];
  const Ray r = lens_ray(cam, lens_target(cam, x, y), x, y, j, seed);
  px_store_ray(rays + 6 * t, r, keys + 3 * t, x, y, j);
}

__global__ __launch_bounds__(PX_BS) void k_pixel_reduce(const CameraDev* __restrict__ camp, int npx, int pre,
                                                         int max_samples, const double* __restrict__ col,
                                                         const int32_t* __restrict__ st, double* __restrict__ rgb,
                                                         double* __restrict__ var_out, int32_t* __restrict__ info,
                                                         int32_t* __restrict__ list, int32_t* __restrict__ count) {
  const size_t i = (size_t)blockIdx.x * PX_BS + threadIdx.x;
  if (i >= (size_t)npx) return;
  const CameraDev& cam = *camp;
  const double* sc = col + 3 * i * (size_t)pre;
  const int32_t* ss = st + i * (size_t)pre;
  int32_t err = 0, at = 0;
  V3 avg = v3(0.0, 0.0, 0.0);
  for (int j = 0; j < pre; j++) {
    avg = vadd(avg, v3(sc[3 * j], sc[3 * j + 1], sc[3 * j + 2]));
    if (!err && ss[j]) {
      err = ss[j];
      at = j;
    }
  }
  double* o = rgb + 3 * i;
  if (err) {                                   // render_at raised at pre sample `at`
    const double qnan = __builtin_nan("");
    px_store3(o, v3(qnan, qnan, qnan));
    if (var_out) var_out[i] = qnan;
    if (info) {
      info[2 * i] = err;
      info[2 * i + 1] = at + 1;
    }
    return;
  }
  avg = vdiv(avg, (double)pre);
  double variance = 0.0;                       // camera.rb:80-85
  for (int j = 0; j < pre; j++) {
    const V3 dd = vsub(v3(sc[3 * j], sc[3 * j + 1], sc[3 * j + 2]), avg);
    double mx = dd.x;
    if (dd.y > mx) mx = dd.y;
    if (dd.z > mx) mx = dd.z;
    variance += mx * mx;                       // .max ** 2
  }
  variance /= (double)pre;
  if (var_out) var_out[i] = variance;
  int samples = pre;
  if (variance >= cam.variant_threshold) {
    if (max_samples > pre) {                   // extra samples: k_pixel_finish ends this pixel, its pre mean parked
      list[atomicAdd(count, 1)] = (int32_t)i;
      samples = max_samples;
    } else {
      avg = vdiv(vadd(vsc(avg, (double)pre), v3(0.0, 0.0, 0.0)), (double)max_samples);
    }
  }
  px_store3(o, avg);
  if (info) {
    info[2 * i] = 0;
    info[2 * i + 1] = samples;
  }
}

// Sized for every pixel of the chunk; the threads past the list leave at once.
__global__ __launch_bounds__(PX_BS) void k_pixel_extra_rays(const CameraDev* __restrict__ camp, uint64_t seed,
                                                             const int32_t* __restrict__ xy, int npx, int pre,
                                                             int n_extra, const int32_t* __restrict__ list,
                                                             int32_t* __restrict__ count, double* __restrict__ rays,
                                                             int32_t* __restrict__ keys) {
  const size_t t = (size_t)blockIdx.x * PX_BS + threadIdx.x;
  const int listed = count[0] < npx ? count[0] : npx;
  if (t == 0) count[1] = listed * n_extra;      // the live ray count of the trace that follows
  const size_t e = t / (size_t)n_extra;
  if (e >= (size_t)listed) return;
  const CameraDev& cam = *camp;
  const int j = pre + (int)(t - e * (size_t)n_extra);
  const size_t i = (size_t)list[e];
  const int x = xy[2 * i], y = xy[2 * i + 1];
  const Ray r = lens_ray(cam, lens_target(cam, x, y), x, y, j, seed);
  px_store_ray(rays + 6 * t, r, keys + 3 * t, x, y, j);
}

__global__ __launch_bounds__(PX_BS) void k_pixel_finish(int npx, int pre, int max_samples,
                                                         const int32_t* __restrict__ list,
                                                         const int32_t* __restrict__ count,
                                                         const double* __restrict__ col, const int32_t* __restrict__ st,
                                                         double* __restrict__ rgb, int32_t* __restrict__ info) {
  const size_t e = (size_t)blockIdx.x * PX_BS + threadIdx.x;
  const int listed = count[0] < npx ? count[0] : npx;
  if (e >= (size_t)listed) return;
  const size_t i = (size_t)list[e];
  const int n_extra = max_samples - pre;
  const double* sc = col + 3 * e * (size_t)n_extra;
  const int32_t* ss = st + e * (size_t)n_extra;
  double* o = rgb + 3 * i;
  const V3 avg = v3(o[0], o[1], o[2]);         // the pre mean parked by k_pixel_reduce
  V3 cv = v3(0.0, 0.0, 0.0);
  int32_t err = 0, at = 0;
  for (int j = 0; j < n_extra; j++) {
    cv = vadd(cv, v3(sc[3 * j], sc[3 * j + 1], sc[3 * j + 2]));
    if (!err && ss[j]) {
      err = ss[j];
      at = j;
    }
  }
  if (err) {                                   // render_at raised at extra sample pre + at (the variance stands)
    const double qnan = __builtin_nan("");
    px_store3(o, v3(qnan, qnan, qnan));
    if (info) {
      info[2 * i] = err;
      info[2 * i + 1] = pre + at + 1;
    }
    return;
  }
  px_store3(o, vdiv(vadd(vsc(avg, (double)pre), cv), (double)max_samples));
}

static unsigned px_grid(size_t n) { return (unsigned)((n + PX_BS - 1) / PX_BS); }

hipError_t launch_pixel_rays(const CameraDev* cam, uint64_t seed, const int32_t* d_xy, int npx, int pre,
                             const PixelBufs& b, hipStream_t s) {
  hipLaunchKernelGGL(k_pixel_rays, dim3(px_grid((size_t)npx * pre)), dim3(PX_BS), 0, s, cam, seed, d_xy, npx, pre,
                     b.rays, b.keys, b.count);
  return hipGetLastError();
}

hipError_t launch_pixel_reduce(const CameraDev* cam, int npx, int pre, int max_samples, const PixelBufs& b,
                               double* d_rgb, double* d_variance, int32_t* d_info, hipStream_t s) {
  hipLaunchKernelGGL(k_pixel_reduce, dim3(px_grid((size_t)npx)), dim3(PX_BS), 0, s, cam, npx, pre, max_samples, b.col,
                     b.st, d_rgb, d_variance, d_info, b.list, b.count);
  return hipGetLastError();
}

hipError_t launch_pixel_extra_rays(const CameraDev* cam, uint64_t seed, const int32_t* d_xy, int npx, int pre,
                                   int max_samples, const PixelBufs& b, hipStream_t s) {
  const int n_extra = max_samples - pre;
  hipLaunchKernelGGL(k_pixel_extra_rays, dim3(px_grid((size_t)npx * n_extra)), dim3(PX_BS), 0, s, cam, seed, d_xy, npx,
                     pre, n_extra, b.list, b.count, b.rays, b.keys);
  return hipGetLastError();
}

hipError_t launch_pixel_finish(int npx, int pre, int max_samples, const PixelBufs& b, double* d_rgb, int32_t* d_info,
                               hipStream_t s) {
  hipLaunchKernelGGL(k_pixel_finish, dim3(px_grid((size_t)npx)), dim3(PX_BS), 0, s, npx, pre, max_samples, b.list,
                     b.count, b.col, b.st, d_rgb, d_info);
  return hipGetLastError();
}

}  // namespace rtx
