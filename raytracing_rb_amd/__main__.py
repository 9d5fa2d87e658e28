"""CLI counterpart of src/main.rb:

    python -m raytracing_rb_amd <s|N|g> <out.png> <world.yml> <camera.yml> [--seed S] [--device D]

``s`` renders on one GPU (Camera#render_sync); ``N`` splits the frame over N
GPU workers (Camera#render_fork); ``g`` writes the geometry passes of camera
sample 0 (normal, depth, albedo) instead.  The reference seeds Random with 1
(main.rb:10); here the seed keys the counter RNG.
"""

import sys


def write_geometry(camera, out_file, max_distance):
    """Mode ``g``: sample 0's first-hit buffers (Camera.first_hit) as three
    pictures, quantized like a colour frame: out.normal.png ((n + 1) / 2),
    out.depth.png (grey, 1 - min(depth / max_distance, 1)), out.albedo.png."""
    import numpy as np
    from . import png
    from .runtime import quantize
    g = camera.first_hit()
    stem = out_file[:-4] if out_file.endswith(".png") else out_file
    depth = 1.0 - np.minimum(g["depth"] / float(max_distance), 1.0)
    frames = {"normal": (g["normal"] + 1.0) / 2.0, "depth": np.repeat(depth[..., None], 3, axis=2),
              "albedo": g["albedo"]}
    for name, fb in frames.items():
        png.write("%s.%s.png" % (stem, name), quantize(fb))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    seed, device = 1, 0
    if "--seed" in argv:
        i = argv.index("--seed")
        seed = int(argv[i + 1])
        del argv[i:i + 2]
    if "--device" in argv:
        i = argv.index("--device")
        device = int(argv[i + 1])
        del argv[i:i + 2]
    if len(argv) != 4:
        print("parameter error")                      # main.rb:5-8
        return 1
    mode, out_file, world_file, camera_file = argv
    from .api import Camera, World
    world = World(world_file)
    camera = Camera(world, camera_file, device=device, seed=seed)
    if mode == "s":
        camera.render_sync(out_file)
    elif mode == "g":
        write_geometry(camera, out_file, world.max_distance)
    else:
        camera.render_fork(out_file, int(mode))
    return 0


if __name__ == "__main__":
    sys.exit(main())
