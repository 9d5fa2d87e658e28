// Host-only check of SPH_BVH_QLDS's 16-bit leaf records (tests/test_qleaf.py): reads "x y z r" lines,
// packs the spheres and builds the hierarchy with rtx_scene_upload's own steps (rtx_scene_build.h;
// median or SAH, argv[1]), quantizes its leaves and prints, per occupied slot, the true sphere and the
// float32 ball the device decodes (fmaf(q, step, org) per axis, q * rstep), as exact hex floats, then
// the scene's q_ok and max_err.
#ifdef __HIPCC__   // (built as a HIP source: rtx_vec3.h's function qualifiers come from the runtime header)
#include <hip/hip_runtime.h>
#endif
#include <iostream>

#include "../raytracing_rb_amd/csrc/rtx_scene_build.h"

int main(int argc, char** argv) {
  using namespace rtx;
  const bool sah = argc > 1 && argv[1][0] == '1';
  HostScene H;
  double c[3], r;
  while (std::cin >> c[0] >> c[1] >> c[2] >> r) pack_sphere(H, (int)H.sph64.size(), c, r);
  build_hierarchy(H, sah, false);
  pack_quantized_leaves(H);
  const Bvh4Builder& b = *H.bb;
  const QuantLeaves& ql = H.ql;
  for (size_t k = 0; k < b.slot64.size(); k++) {
    const Sphere64& s = b.slot64[k];
    if (!(s.r >= 0.0)) continue;
    const uint32_t* w = ql.rec.data() + (k / BVH_LEAF) * 8;
    const int h = (int)(k % BVH_LEAF);
    auto q = [&](int comp) { return (w[comp * 2 + h / 2] >> (16 * (h % 2))) & 0xffffu; };
    const float dx = std::fmaf((float)q(0), ql.step[0], ql.org[0]), dy = std::fmaf((float)q(1), ql.step[1], ql.org[1]),
                dz = std::fmaf((float)q(2), ql.step[2], ql.org[2]), dr = (float)q(3) * ql.rstep;
    printf("%a %a %a %a %a %a %a %a\n", s.c[0], s.c[1], s.c[2], s.r, (double)dx, (double)dy, (double)dz, (double)dr);
  }
  printf("ok %d %a %a\n", ql.ok ? 1 : 0, ql.max_err, (double)H.dev.sph_scale);
  return 0;
}
