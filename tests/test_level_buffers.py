"""The bounce-level engine's batch and buffer layout (csrc/rtx_batch.h), on the host.

Both entries of the engine (rtx_render_device -> render_levels, rtx_trace_device ->
trace_levels) take their capacities and the offset of every buffer of their one
allocation from rtx_batch.h; tools/scene_dump.cpp --buffers prints what that header
computes.  Here the tool is held, field by field, to the arithmetic those two
functions (and lv_sort_from, lv_paths32, lv_frame_items, levels_rec_bytes) carried
themselves at commit f136f77, written out again below in Python: `parent_render`
and `parent_trace` follow that commit's statements in their order, so that they can
be read against it.  A capacity rule that changes has to change here too.

The cases are the smallest at which each branch of the arithmetic can go wrong.
For every case that is not refused the layout is also checked on its own terms:
every buffer starts 256-aligned, the buffers follow in order without overlap, and
the last set and the tail end within the total.
"""
import subprocess

import pytest

import plan_scenes

# ---------------------------------------------------------------- the constants at f136f77 (rtx_launch.h, rtx_plan.h)
LV_MAXL, LV_SLICES, LV_CLAIMS, LV_DONE, LV_BINS = 64, 64, 16, 16, 8 << 12
RAY_BYTES, LV_HIT_BYTES, LV_SPLIT_MAX_LIGHTS = 96, 64, 16
UINT32_MAX = 2 ** 32 - 1
# sizeof(LevelCtl): from a static_assert compiled against that commit's rtx_launch.h.  Every field is a
# uint32_t: 4 + 27 words, sc and sh, claim, lay_cnt / lay_pex / lay_cin, lay_base and done, done_sub.
SIZEOF_LEVELCTL = 1648780
assert SIZEOF_LEVELCTL == 4 * (4 + 27 + 2 * (LV_MAXL + 1) * LV_SLICES * 32 + 3 * (LV_MAXL + 1) * LV_CLAIMS * 32 +
                               3 * (LV_MAXL + 2) * LV_SLICES + 2 * (LV_MAXL + 2) + (LV_MAXL + 1) * LV_DONE * 32)

BUFS = ("ctl", "redo_of", "redo_list", "redo_smp", "stage0", "stage1", "rec", "hit", "area", "hlq", "key", "perm", "bins",
        "sorted")
OPTS = ("lv_batch", "lv_stage_pct", "lv_rec_pct", "lv_floor", "lv_streams", "lv_split", "lv_hl_cap", "lv_sort", "lv_sort_from",
        "lv_sort_copy", "lv_ray_bytes")
DEFAULTS = dict(lv_batch=1 << 24, lv_stage_pct=300, lv_rec_pct=1600, lv_floor=1 << 20, lv_streams=2, lv_split=0, lv_hl_cap=0,
                lv_sort=-1, lv_sort_from=0, lv_sort_copy=0, lv_ray_bytes=0)    # the context's defaults at that commit
REFUSE_RECORDS = "bounce-level buffers exceed 2^31 records: lower lv_batch"
REFUSE_PATHS = "lv_ray_bytes 80: this camera's ray paths need 64 bits ((pt + 3)^trace_depth > 2^32)"


def al256(b):
    return (b + 255) & ~255


def levels_rec_bytes(n_light):
    return (8 + 24 * max(n_light, 1) + 15) & ~15


def lv_paths32(c):
    v = 1
    for _ in range(c["depth"]):
        v *= c["pt"] + 3
        if v > 1 << 32:
            return False
    return True


def lv_sort_from(c, n0):
    split = c["lv_split"] != 0 and c["n_light"] <= LV_SPLIT_MAX_LIGHTS
    if c["lv_sort"] == 0 or split:
        return 0
    large = c["n_sphere"] > 512
    if c["lv_sort"] == -1 and c["lv_sort_from"] == 0 and not large and n0 < 1 << 22:
        return 0
    frm = c["lv_sort_from"] if c["lv_sort_from"] > 0 else 1 if large else c["depth"] - 1
    return frm if 1 <= frm < c["depth"] else 0


def _carved(sizes, present):
    """The pointer walk both functions did: every buffer at the sum of the sizes before it."""
    out, at = {}, 0
    for name in BUFS:
        out["off_" + name], out["size_" + name], out["present_" + name] = at, sizes[name], int(present[name])
        at += sizes[name]
    return out, at


def parent_render(c):
    """render_levels (rtx_capi.cpp:670-819 at f136f77)."""
    npx, tiles = c["n"], c["tiles"]
    per_tile = 64 * c["pre"]
    parts = max(1, min(c["lv_streams"], tiles))
    batch_tiles = max(1, min(c["lv_batch"] // per_tile, (tiles + parts - 1) // parts))
    n0 = max(batch_tiles * per_tile, max(0, c["max_samples"] - c["pre"]))
    out = dict(parts=parts, batch_tiles=batch_tiles, n0=n0)
    fl = c["lv_floor"]
    want = max(max(64, fl), n0 * c["lv_stage_pct"] // 100)
    lcap = max(max(n0, 4 * fl), n0 * c["lv_rec_pct"] // 100)
    slog2 = 0
    while (LV_SLICES << slog2) < want:
        slog2 += 1
    scap = LV_SLICES << slog2
    if scap > UINT32_MAX // 2 or lcap > UINT32_MAX // 2:
        return dict(out, refusal=REFUSE_RECORDS)
    path32 = lv_paths32(c)
    if c["lv_ray_bytes"] == 80 and not path32:
        return dict(out, refusal=REFUSE_PATHS)
    rec_bytes = levels_rec_bytes(c["n_light"])
    hlcap = c["lv_hl_cap"] if c["lv_hl_cap"] > 0 else max(4096, lcap // 256)
    sz = dict(hlq=al256(hlcap * 64), ctl=al256(SIZEOF_LEVELCTL), redo_of=al256(n0 * 4), redo_list=al256(n0 * 4),
              redo_smp=al256(n0 * 32), stage0=al256(scap * RAY_BYTES), stage1=al256(scap * RAY_BYTES),
              rec=al256(lcap * rec_bytes))
    sz_extra = al256((npx + 64) * 4)
    split = c["lv_split"] != 0 and c["n_light"] <= LV_SPLIT_MAX_LIGHTS
    hlog2 = 0
    while (LV_SLICES << hlog2) < max(n0, scap):
        hlog2 += 1
    hcap = LV_SLICES << hlog2
    sz["hit"] = al256(hcap * LV_HIT_BYTES) if split else 0
    sz["area"] = al256(hcap * max(1, c["n_light"]) * 16) if split else 0
    sort_from = lv_sort_from(c, n0)
    sort = sort_from > 0
    sz["key"], sz["perm"] = (al256(scap * 2) if sort else 0), (al256(scap * 8) if sort else 0)
    sz["bins"] = al256(LV_BINS * 8) if sort else 0
    sort_copy = sort and c["lv_sort_copy"] == 1
    sz["sorted"] = sz["stage0"] if sort_copy else 0
    set_ = (sz["ctl"] + 2 * sz["redo_of"] + sz["redo_smp"] + 2 * sz["stage0"] + sz["rec"] + sz["hit"] + sz["area"] +
            sz["hlq"] + sz["key"] + sz["perm"] + sz["bins"] + sz["sorted"])
    total = parts * set_ + sz_extra
    present = dict.fromkeys(BUFS, True)           # the carve lambda: null pointers for what the call does not use
    present.update(hit=split, area=split, key=sort, perm=sort, bins=sort, sorted=sort_copy)
    carved, end = _carved(sz, present)
    assert end == set_
    out.update(carved, refusal="-", scap=scap, slog2=slog2, lcap=lcap, hcap=hcap, hlog2=hlog2, hlcap=hlcap,
               rec_bytes=rec_bytes, sort_from=sort_from, sort_copy=int(sort_copy), split=int(split),
               ray_dbl=12 if c["lv_ray_bytes"] == 96 or not path32 else 10, set=set_, tail=sz_extra, total=total)
    return out


def parent_trace(c):
    """trace_levels (rtx_capi.cpp:1645-1720 at f136f77): one part, p.lv_split = 0, p.lv_hslice_log2 = 0,
    p.lv_ray_dbl = 12, and 256 bytes after the set for the extra count that k_level_begin zeroes."""
    levels = bool(c["levels"])
    n0 = max(1, min(c["lv_batch"], c["n"]))
    out = dict(parts=1, batch_tiles=0, n0=n0)
    fl = c["lv_floor"]
    want = max(max(64, fl), n0 * c["lv_stage_pct"] // 100)
    lcap = max(max(n0, 4 * fl), n0 * c["lv_rec_pct"] // 100)
    slog2 = 0
    while (LV_SLICES << slog2) < want:
        slog2 += 1
    scap = LV_SLICES << slog2
    if levels and (scap > UINT32_MAX // 2 or lcap > UINT32_MAX // 2):
        return dict(out, refusal=REFUSE_RECORDS)
    rec_bytes = levels_rec_bytes(c["n_light"])
    hlcap = c["lv_hl_cap"] if c["lv_hl_cap"] > 0 else max(4096, lcap // 256)
    sort_from = lv_sort_from(c, n0) if levels else 0
    sort = sort_from > 0
    sort_copy = sort and c["lv_sort_copy"] == 1
    sz = dict(ctl=al256(SIZEOF_LEVELCTL), redo_of=al256(n0 * 4), redo_list=al256(n0 * 4), redo_smp=al256(n0 * 32),
              stage0=al256(scap * RAY_BYTES) if levels else 0, rec=al256(lcap * rec_bytes) if levels else 0,
              hlq=al256(hlcap * 64) if levels else 0, key=al256(scap * 2) if sort else 0,
              perm=al256(scap * 8) if sort else 0, bins=al256(LV_BINS * 8) if sort else 0, hit=0, area=0)
    sz["stage1"] = sz["stage0"]
    sz["sorted"] = sz["stage0"] if sort_copy else 0
    total = (sz["ctl"] + 2 * sz["redo_of"] + sz["redo_smp"] + 2 * sz["stage0"] + sz["rec"] + sz["hlq"] + sz["key"] +
             sz["perm"] + sz["bins"] + sz["sorted"] + 256)
    present = dict.fromkeys(BUFS, True)           # (lv_stage and lv_rec are set whatever `levels` says; lv_hit and
    present.update(hit=False, area=False, hlq=levels, key=sort, perm=sort, bins=sort, sorted=sort_copy)   # lv_area stay null)
    carved, end = _carved(sz, present)
    assert end + 256 == total                     # p.extra_count: right after the last buffer
    out.update(carved, refusal="-", scap=scap, slog2=slog2, lcap=lcap, hcap=LV_SLICES << 0, hlog2=0,
               hlcap=hlcap if levels else 0,      # p.lv_hlq_cap
               rec_bytes=rec_bytes, sort_from=sort_from, sort_copy=int(sort_copy), split=0, ray_dbl=12, set=end, tail=256,
               total=total)
    return out


def parent_frame_items(c, width, height):
    """lv_frame_items (rtx_capi.cpp:648-654 at f136f77), the third copy, for option lv_sort_effective."""
    tiles = ((width + 7) // 8) * ((height + 7) // 8)
    per_tile = 64 * max(1, c["pre"])
    parts = max(1, min(c["lv_streams"], tiles))
    batch_tiles = max(1, min(c["lv_batch"] // per_tile, (tiles + parts - 1) // parts))
    return max(batch_tiles * per_tile, max(0, c["max_samples"] - c["pre"]))


# ---------------------------------------------------------------- the cases
def render(tiles, npx=None, **kw):
    c = dict(DEFAULTS, trace=0, tiles=tiles, n=tiles * 64 if npx is None else npx, pre=1, max_samples=1, depth=3, pt=1,
             n_sphere=64, n_light=1, levels=1)
    assert not set(kw) - set(c), kw
    return dict(c, **kw)


def trace(nrays, **kw):
    return dict(render(0, **kw), trace=1, n=nrays)


SMALL = dict(lv_floor=0, lv_streams=1)             # the floors out of the way: capacities follow n0
CASES = {
    "defaults, the C2 frame": render(32400, 1920 * 1080, pre=4, max_samples=4, depth=5),
    "defaults, a 48 x 27 frame with extra samples": render(24, 48 * 27, pre=2, max_samples=3),
    # want against the slices
    "want = 64 << 6 (floor)": render(1, lv_floor=4096, lv_streams=1),
    "want = (64 << 6) + 1 (floor)": render(1, lv_floor=4097, lv_streams=1),
    "want = 64 << 6 (items)": render(100, lv_stage_pct=64, **SMALL),
    "want = (64 << 6) + 1 (rays)": trace(4097, lv_stage_pct=100, lv_floor=0),
    "the floor of 64 slots binds": render(1, lv_stage_pct=1, **SMALL),
    # lcap: the sides of its maxima
    "lcap from lv_rec_pct 101": render(100, lv_rec_pct=101, **SMALL),
    "lcap from n0 (lv_rec_pct 50)": render(100, lv_rec_pct=50, **SMALL),
    "lcap from 4 x the default floor": render(100, lv_rec_pct=101, lv_streams=1),
    # n0
    "n0 from the extra samples": render(1, max_samples=100, **SMALL),
    "n0 from the tiles, extra samples below": render(2, pre=2, max_samples=100, **SMALL),
    "lv_batch below one tile": render(9, lv_batch=32, **SMALL),
    "lv_batch of three tiles": render(9, pre=2, lv_batch=3 * 128 + 127, **SMALL),
    # split phases
    "split on at 16 lights": render(9, n_light=16, lv_split=1),
    "split ignored at 17 lights": render(9, n_light=17, lv_split=1),
    "split, hcap from n0": render(100, lv_split=1, lv_stage_pct=50, **SMALL),
    "split, hcap from scap": render(100, lv_split=1, lv_stage_pct=300, **SMALL),
    "split without lights": render(9, n_light=0, lv_split=1),
    # binning: the batch size, the first level, the copy
    "2^22 - 64 samples bin nothing": render(65535, lv_streams=1),
    "2^22 samples bin the last level": render(65536, lv_streams=1),
    "2^22 - 1 rays bin nothing": trace((1 << 22) - 1),
    "2^22 rays bin the last level": trace(1 << 22),
    "lv_sort_from = depth": render(9, lv_sort=1, lv_sort_from=3),
    "lv_sort_from = depth - 1": render(9, lv_sort=1, lv_sort_from=2),
    "lv_sort_from 1 below 2^22 under auto": render(9, lv_sort_from=1),
    "lv_sort_copy on": render(9, lv_sort=1, lv_sort_copy=1),
    "lv_sort_copy off": render(9, lv_sort=1, lv_sort_copy=0),
    "lv_sort_copy without binning": render(9, lv_sort=0, lv_sort_copy=1),
    "binning and split asked together": render(9, lv_sort=1, lv_split=1),
    "depth 1 has no level to bin": render(9, lv_sort=1, depth=1),
    # auto against explicit
    "lv_hl_cap 5": render(9, lv_hl_cap=5),
    "lv_hl_cap auto above its 4096": render(100, lv_rec_pct=20000, pre=4, max_samples=4, **SMALL),
    # refusals
    "refused: 2^31 staged records": render(9, lv_floor=1 << 31),
    "refused: 2^31 tree records": render(9, lv_floor=1 << 29),
    "just below the refusals": render(9, lv_floor=(1 << 29) - 1),
    "trace refused: 2^31 tree records": trace(64, lv_floor=1 << 29),
    "trace through the lanes engine is not": trace(64, levels=0, lv_floor=1 << 29),
    # trace calls
    "trace, split asked (levels)": trace(64, lv_split=1, lv_sort=1),
    "trace, split asked (lanes)": trace(64, levels=0, lv_split=1, lv_sort=1),
    "trace, 17 lights and split asked": trace(64, n_light=17, lv_split=1, lv_sort=1),
    "trace, lv_hl_cap 5 (lanes)": trace(64, levels=0, lv_hl_cap=5),
    "trace, binning with the copy": trace(64, lv_sort=1, lv_sort_copy=1),
}
for streams in (1, 2, 3, 4):                       # parts: more tiles than parts, and fewer (or as many)
    CASES["lv_streams %d, 9 tiles" % streams] = render(9, lv_streams=streams, lv_floor=0)
    CASES["lv_streams %d, 1 tile" % streams] = render(1, lv_streams=streams, lv_floor=0)
    CASES["lv_streams %d, %d tiles" % (streams, max(1, streams - 1))] = render(max(1, streams - 1), lv_streams=streams)
for sort in (-1, 0, 1):
    for spheres in (512, 513):
        CASES["lv_sort %d, %d spheres" % (sort, spheres)] = render(9, lv_sort=sort, n_sphere=spheres, depth=4)
for depth in (8, 9):                               # pt 13: (pt + 3)^depth is 2^32 at depth 8, above it at 9
    for rb in (0, 80, 96):
        CASES["lv_ray_bytes %d, 16^%d paths" % (rb, depth)] = render(9, pt=13, depth=depth, lv_ray_bytes=rb)
    CASES["trace, lv_ray_bytes 80, 16^%d paths" % depth] = trace(64, pt=13, depth=depth, lv_ray_bytes=80)
for levels in (1, 0):
    for nrays in (1, 63, 64, 65, 1000, 1001):      # lv_batch 1000: the batch and one ray more
        CASES["trace %d rays, levels %d" % (nrays, levels)] = trace(nrays, levels=levels, lv_batch=1000, lv_floor=0)
NAMES = list(CASES)


def case_line(c):
    return " ".join(str(c[k]) for k in ("trace", "tiles", "n", "pre", "max_samples", "depth", "pt", "n_sphere", "n_light",
                                        "levels") + OPTS)


@pytest.fixture(scope="module")
def dumped(tmp_path_factory):
    """The tool's line per case, as {name: value}, from one run (cases on stdin)."""
    exe = plan_scenes.build_tool(tmp_path_factory.mktemp("scene_dump"))
    p = subprocess.run([exe, "--buffers"], input="".join(case_line(CASES[n]) + "\n" for n in NAMES), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 0, (p.stdout, p.stderr)
    lines = p.stdout.splitlines()
    assert len(lines) == len(NAMES), p.stdout
    out = {}
    for name, line in zip(NAMES, lines):
        f = line.split()
        out[name] = {k: (v if k == "refusal" else int(v)) for k, v in zip(f[0::2], f[1::2])}
    return out


def expected(c):
    return parent_trace(c) if c["trace"] else parent_render(c)


def test_the_table_reaches_every_branch():
    """What the cases are there for, said of the second statement alone."""
    e = {n: expected(CASES[n]) for n in NAMES}
    ok = {n: v for n, v in e.items() if v["refusal"] == "-"}
    assert sorted(v["refusal"] for v in e.values() if v["refusal"] != "-") == [REFUSE_RECORDS] * 3 + [REFUSE_PATHS]
    assert e["want = 64 << 6 (floor)"]["slog2"] == 6 and e["want = (64 << 6) + 1 (floor)"]["slog2"] == 7
    assert e["want = 64 << 6 (items)"]["scap"] == 4096 and e["want = (64 << 6) + 1 (rays)"]["scap"] == 8192
    assert e["the floor of 64 slots binds"]["scap"] == 64
    assert e["lcap from lv_rec_pct 101"]["lcap"] == 6464 and e["lcap from n0 (lv_rec_pct 50)"]["lcap"] == 6400
    assert e["lcap from 4 x the default floor"]["lcap"] == 4 << 20
    assert e["n0 from the extra samples"]["n0"] == 99 and e["n0 from the tiles, extra samples below"]["n0"] == 256
    assert e["lv_batch below one tile"]["batch_tiles"] == 1 and e["lv_batch of three tiles"]["batch_tiles"] == 3
    assert {v["parts"] for v in ok.values()} == {1, 2, 3, 4}
    assert e["split on at 16 lights"]["split"] == 1 and e["split ignored at 17 lights"]["split"] == 0
    assert e["split, hcap from n0"]["hcap"] == 8192 > e["split, hcap from n0"]["scap"]
    assert e["split, hcap from scap"]["hcap"] == e["split, hcap from scap"]["scap"] == 32768
    assert [e["lv_sort %d, %d spheres" % k]["sort_from"] for k in ((-1, 512), (-1, 513), (0, 513), (1, 512), (1, 513))] == \
        [0, 1, 0, 3, 1]
    assert e["2^22 - 64 samples bin nothing"]["sort_from"] == 0 and e["2^22 samples bin the last level"]["sort_from"] == 2
    assert e["2^22 - 1 rays bin nothing"]["sort_from"] == 0 and e["2^22 rays bin the last level"]["sort_from"] == 2
    assert e["lv_sort_from = depth"]["sort_from"] == 0 and e["lv_sort_from = depth - 1"]["sort_from"] == 2
    assert e["lv_sort_copy on"]["size_sorted"] > 0 and e["lv_sort_copy off"]["size_sorted"] == 0
    assert e["lv_hl_cap 5"]["hlcap"] == 5 and e["lv_hl_cap auto above its 4096"]["hlcap"] == 20000
    assert [e["lv_ray_bytes %d, 16^%d paths" % k].get("ray_dbl") for k in ((0, 8), (80, 8), (96, 8), (0, 9), (80, 9), (96, 9))] \
        == [10, 10, 12, 12, None, 12]
    assert e["trace, split asked (levels)"]["size_hit"] == 0 and e["trace, split asked (levels)"]["sort_from"] == 0
    assert e["trace, 17 lights and split asked"]["sort_from"] == 2
    assert e["trace 1001 rays, levels 1"]["n0"] == 1000 and e["trace 1 rays, levels 0"]["size_rec"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_the_header_computes_what_both_entries_did(dumped, name):
    got, want = dumped[name], expected(CASES[name])
    assert got.pop("sizeof_LevelCtl") == SIZEOF_LEVELCTL
    if want["refusal"] != "-":                     # a refused call: its items and the reason, no layout
        assert {k: got[k] for k in want} == dict(want, refusal=want["refusal"].replace(" ", "_"))
        return
    assert sorted(got) == sorted(want)
    diff = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not diff, diff


@pytest.mark.parametrize("name", NAMES)
def test_buffers_are_aligned_ordered_and_within_the_total(dumped, name):
    g = dumped[name]
    if g["refusal"] != "-":
        return
    end = 0
    for b in BUFS:
        assert g["off_" + b] % 256 == 0 and g["size_" + b] % 256 == 0, b
        assert g["off_" + b] >= end, b             # after the one before it
        end = g["off_" + b] + g["size_" + b]
    assert end <= g["set"] and g["set"] % 256 == 0
    assert g["parts"] * g["set"] + g["tail"] <= g["total"]
    # the tail holds the extra count's 64 words and, for a render, the list of the region's pixels
    assert g["tail"] >= (256 if CASES[name]["trace"] else (CASES[name]["n"] + 64) * 4)
    # what the kernels index: a buffer that is present holds its capacity
    n0, levels = g["n0"], CASES[name]["levels"]
    need = dict(ctl=SIZEOF_LEVELCTL, redo_of=n0 * 4, redo_list=n0 * 4, redo_smp=n0 * 32,
                stage0=g["scap"] * 8 * g["ray_dbl"] * levels, stage1=g["scap"] * 8 * g["ray_dbl"] * levels,
                rec=g["lcap"] * g["rec_bytes"] * levels, hit=g["hcap"] * LV_HIT_BYTES,
                area=g["hcap"] * max(1, CASES[name]["n_light"]) * 16, hlq=g["hlcap"] * 64, key=g["scap"] * 2,
                perm=g["scap"] * 8, bins=LV_BINS * 8, sorted=g["scap"] * 8 * g["ray_dbl"])
    for b in BUFS:
        if g["present_" + b]:
            assert g["size_" + b] >= need[b], b
        else:
            assert g["size_" + b] == 0, b


@pytest.mark.parametrize("width,height,pre,max_samples,streams", [(1920, 1080, 4, 4, 2), (1920, 1080, 4, 4, 1), (48, 27, 2, 3, 2),
                                                                  (8, 8, 1, 100, 4), (9, 9, 16, 16, 3)])
def test_the_frame_items_of_lv_sort_effective(width, height, pre, max_samples, streams):
    """lv_frame_items, the third copy, is batch_items over the frame's tiles (pre >= 1: rtx_camera_set)."""
    c = render(((width + 7) // 8) * ((height + 7) // 8), width * height, pre=pre, max_samples=max_samples, lv_streams=streams)
    assert parent_frame_items(c, width, height) == parent_render(c)["n0"]
