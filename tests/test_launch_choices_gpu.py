"""Lowered applies on every launch configuration the tuners can pick, at sizes where the launcher's own rules apply.

Every apply of 2^24 cells or more tunes itself on first use (apply_launch.hpp launch_apply / tune_apply), and the
plan-time tuner (neptune_hip_autotune_fn) does the same on request: a lowered body can then run on any default march
tile with any chunk length either tuner tries.  This module runs them all, on generated footprints:

  * the sweep: each family's geometry-level entry on the direct kernel (both forms), the automatic tile and chunk, every
    tile crossed with every tuner chunk length (clamped to the plane count) and the interior + two-edge region split,
    every result bit for bit against the direct one on the device, every launch checked through neptune_hip_last_launch
    (no silent fallback), the direct result against the numpy oracle;
  * in child processes: the lowered 1024^3 headline (and 27-point 512^3, 5-point 8192^2) on its tuned choice, and the
    tuners' own picks for the sweep's families, each inside what the sweep ran;
  * the launch-choice key (input boxes relative to the result) and the aliasing refusal of the geometry entries.

The chunk lists and the tile table are read from the tuners' source, so a length or tile added there is swept here.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import helpers
from helpers import bits_equal, mismatch_report, oracle

REPO = helpers.REPO
LAUNCH_HPP = REPO / "neptune-pde-solver_amd" / "csrc" / "kernels" / "apply_launch.hpp"
RT_HIP = REPO / "neptune-pde-solver_amd" / "csrc" / "runtime" / "neptune_hip_rt.hip"


# ---- the tuners' candidates, read from their source ---------------------------------------------------------------
def tuner_chunk_lists():
    """{"first_use": {"chunks3": [...], "chunks2": [...]}, "plan_time": {...}}: the chunk lengths tune_apply
    (apply_launch.hpp) and autotune_launches (neptune_hip_rt.hip) try; 0 = the automatic chunk"""
    out = {}
    for name, path in (("first_use", LAUNCH_HPP), ("plan_time", RT_HIP)):
        found = {}
        for m in re.finditer(r"\b(chunks[23])\[\]\s*=\s*\{([^}]*)\}", path.read_text()):
            found[m.group(1)] = [int(x) for x in m.group(2).split(",") if x.strip()]
        out[name] = found
    return out


def default_tiles(rank):
    """rows of NEPTUNE_MARCH<rank>_DEFAULT as dicts (index, jk, name): the tiles every lowered module holds"""
    text = LAUNCH_HPP.read_text()
    m = re.search(rf"#define NEPTUNE_MARCH{rank}_DEFAULT\(X\)((?:[^\n]*\\\n)+[^\n]*)", text)
    if not m:
        return []
    rows = []
    for args in re.findall(r"\bX\(([^)]*)\)", m.group(1)):
        f = [a.strip() for a in args.split(",")]
        rows.append({"index": int(f[0]), "jk": f[9] == "true", "name": f[-1].strip('"')})
    return rows


def tuner_lengths():
    """every positive chunk length either tuner tries, for either rank"""
    lists = tuner_chunk_lists()
    return sorted({c for per in lists.values() for lst in per.values() for c in lst if c > 0})


def test_tuner_sources_parse():
    """host side: the parser finds both tuners' chunk lists and both default tile tables; if either source changes
    shape, this fails instead of the GPU sweep silently sweeping nothing"""
    lists = tuner_chunk_lists()
    for name in ("first_use", "plan_time"):
        assert lists[name].get("chunks3"), (name, lists)
        assert all(c >= 0 for lst in lists[name].values() for c in lst), (name, lists)
        assert any(c > 0 for c in lists[name]["chunks3"]), (name, lists)
    assert lists["first_use"].get("chunks2") and all(c > 0 for c in lists["first_use"]["chunks2"]), lists
    assert all(c > 0 for c in lists["first_use"]["chunks3"]), lists
    assert 0 in lists["plan_time"]["chunks3"], lists          # the plan-time tuner also times the automatic chunk
    for rank in (3, 2):
        rows = default_tiles(rank)
        assert len(rows) > 0, rank
        assert [r["index"] for r in rows] == list(range(len(rows))), rows
    assert [r["jk"] for r in default_tiles(3)] == [False] * len(default_tiles(3))
    assert any(r["jk"] for r in default_tiles(2)) and not all(r["jk"] for r in default_tiles(2))
    assert 512 in tuner_lengths() and 32 in tuner_lengths()


# ---- families ----------------------------------------------------------------------------------------------------
def _stencil_text(kind):
    import make_stencil_mlir

    def text(out_box, bounds, in_boxes):
        shape = [u - l for l, u in zip(*out_box)]
        return make_stencil_mlir.stencil_module(kind, shape, origin=list(out_box[0]), bounds=bounds)
    return text


def _own_text(elem, accesses):
    from test_ownbox_gpu import module_text

    def text(out_box, bounds, in_boxes):
        return module_text(elem, out_box, bounds, in_boxes, accesses)
    return text


def _halo_text(elem, nin, accesses):
    """test_multihalo_gpu's generator (every input in the result's box, logical origin 0; coefficients for up to 168
    taps): a box elsewhere is moved to the origin -- the body's only index term is the last index, which no slab moves"""
    from test_multihalo_gpu import module_text

    def text(out_box, bounds, in_boxes):
        assert all(b == out_box for b in in_boxes) and out_box[0][-1] == 0
        shape = [u - l for l, u in zip(*out_box)]
        lb = [b - o for b, o in zip(bounds[0], out_box[0])]
        ub = [b - o for b, o in zip(bounds[1], out_box[0])]
        return module_text(shape, elem, nin, accesses, lb, ub)
    return text


def _star(rank, r):
    from test_ownbox_gpu import star
    return star(rank, r)


def _box(shape, lb=None):
    lb = [0] * len(shape) if lb is None else list(lb)
    return (lb, [a + n for a, n in zip(lb, shape)])


class Geometry:
    def __init__(self, shape, bounds, in_boxes=None, auto_tile=None):
        self.out_box = _box(shape)
        self.shape = tuple(shape)
        self.bounds = (list(bounds[0]), list(bounds[1]))
        self.in_boxes = in_boxes            # None: every input in the result's box
        self.auto_tile = auto_tile          # the tile pick_march_variant lands on (asserted through last_launch)

    def boxes(self, nin):
        return [self.out_box] + [self.out_box if self.in_boxes is None else self.in_boxes[k] for k in range(1, nin)]


class Family:
    def __init__(self, name, rank, elem, function, nin, radius, text, geoms, nacc, tile2_only=False):
        self.name, self.rank, self.elem, self.function, self.nin = name, rank, elem, function, nin
        self.radius, self.text, self.geoms, self.nacc, self.tile2_only = radius, text, geoms, nacc, tile2_only

    def module_text(self, geo):
        return self.text(geo.out_box, geo.bounds, geo.boxes(self.nin))


def _families():
    s3, s2 = _star(3, 1), _star(2, 1)
    # a radius-2 box footprint: corners, edges and faces of the 5x5x5 cube
    box2 = [(a, b, c) for a in (-2, 0, 2) for b in (-2, 0, 2) for c in (-2, 0, 2) if (a, b, c) != (0, 0, 0) and (a == 0) + (b == 0) + (c == 0) != 1]
    box2 += [(1, -1, 1), (-1, 1, -1), (2, 1, 0), (0, -2, 1)]
    f = [
        Family("7pt_f64", 3, "f64", "lap3d", 1, 1, _stencil_text("3d7"), [
            # more planes than the longest chunk, 2^k+1 rows (row-tail trim), two K tiles of tile 0, bounds two rows in
            Geometry((600, 129, 512), ([1, 1, 1], [599, 127, 511]), auto_tile=0),
            Geometry((300, 256, 512), ([1, 1, 1], [299, 255, 511]), auto_tile=4),      # from 256 rows: the 64-row tile
        ], 7),
        Family("27pt_f32", 3, "f32", "lap27", 1, 1, _stencil_text("3d27"), [
            Geometry((257, 129, 520), ([1, 2, 1], [256, 128, 519]), auto_tile=3),      # small for a box: the small tile
        ], 27),
        Family("star2_f64", 3, "f64", "resid", 1, 2, _own_text("f64", [(0, (0, 0, 0))] + [(0, o) for o in _star(3, 2)]), [
            Geometry((257, 129, 520), ([2, 2, 3], [255, 127, 518]), auto_tile=7),
        ], 13),
        Family("star4_f64", 3, "f64", "resid", 1, 4, _own_text("f64", [(0, (0, 0, 0))] + [(0, o) for o in _star(3, 4)]), [
            # ragged rows with a K radius of two lane vectors (ragged_extra_vectors)
            Geometry((257, 129, 521), ([4, 4, 4], [253, 124, 517]), auto_tile=7),
        ], 25),
        Family("star8_f32", 3, "f32", "resid", 1, 8, _halo_text("f32", 1, [(0, (0, 0, 0))] + [(0, o) for o in _star(3, 8)]), [
            Geometry((257, 129, 1030), ([8, 8, 8], [249, 121, 1021]), auto_tile=7),
        ], 49),
        Family("box2_f32", 3, "f32", "resid", 1, 2, _own_text("f32", [(0, (0, 0, 0))] + [(0, o) for o in box2]), [
            Geometry((257, 257, 1024), ([2, 2, 2], [255, 254, 1022]), auto_tile=2),
        ], 1 + len(box2)),
        Family("pair2_f64", 3, "f64", "resid", 2, 2,
               _own_text("f64", [(0, (0, 0, 0))] + [(0, o) for o in _star(3, 2)] + [(1, (0, 0, 0))] + [(1, o) for o in _star(3, 2)]), [
            Geometry((257, 129, 520), ([2, 3, 2], [255, 127, 518]), auto_tile=7),
        ], 26),
        # input 0 read at the centre, input 1 -- a 7-point star -- in a box of its own, wider along J and K
        Family("ownbox_f64", 3, "f64", "resid", 2, 1,
               _own_text("f64", [(0, (0, 0, 0)), (1, (0, 0, 0))] + [(1, o) for o in s3]), [
            Geometry((300, 129, 320), ([1, 0, 0], [299, 129, 320]), in_boxes=[None, ([0, -1, -2], [300, 131, 323])], auto_tile=1),
        ], 8),
        Family("5pt_f64", 2, "f64", "lap2d", 1, 1, _stencil_text("2d5"), [
            Geometry((1025, 1031), ([1, 1], [1024, 1029]), auto_tile=0),
        ], 5),
        Family("star4_2d_f64", 2, "f64", "resid", 1, 4, _own_text("f64", [(0, (0, 0))] + [(0, o) for o in _star(2, 4)]), [
            Geometry((1025, 1031), ([4, 4], [1020, 1027]), auto_tile=1),
        ], 17, tile2_only=True),
        Family("pair_2d_f64", 2, "f64", "resid", 2, 1,
               _own_text("f64", [(0, (0, 0))] + [(0, o) for o in s2] + [(1, (0, 0))] + [(1, o) for o in s2]), [
            Geometry((1025, 1031), ([1, 2], [1024, 1030]), auto_tile=2),
        ], 10),
    ]
    return {fam.name: fam for fam in f}


FAMILIES = _families()


def swept_chunks(planes):
    """what a tuner's chunk length becomes on `planes` planes (longer ones clamp to the plane count), plus 0"""
    return sorted({0} | {min(c, planes) for c in tuner_lengths()})


# ---- device side -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nh(built_libs, tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    os.environ["NEPTUNE_CACHE_DIR"] = str(tmp_path_factory.mktemp("neptune_cache"))
    from neptune_hip import _capi, apply, fields, lowering
    lib = _capi.load()
    lib.neptune_hip_init(0)
    helpers.prefetch_modules([fam.module_text(g) for fam in FAMILIES.values() for g in fam.geoms])

    class NS:
        pass
    ns = NS()
    ns.torch, ns.capi, ns.apply, ns.fields, ns.lowering, ns.lib = torch, _capi, apply, fields, lowering, lib
    return ns


def _dtype(nh, elem):
    return nh.capi.F64 if elem == "f64" else nh.capi.F32


def _last(nh):
    cfg = nh.capi.LaunchCfg()
    assert nh.lib.neptune_hip_last_launch(C.byref(cfg)) == 1
    return cfg.kernel, cfg.variant, cfg.chunk


def _host_part(field, box):
    """the cells of `box` (logical) of a device field, on the host"""
    sl = tuple(slice(a - f, b - f) for a, b, f in zip(box[0], box[1], field.lb))
    return field.tensor[sl].cpu().numpy()


def oracle_part(fam, geo, ins, d, lo, hi):
    """the oracle's result on result-physical range [lo, hi) along dim d (every cell of the other dims): the module
    text re-emitted for a slab of the boxes wide enough for the footprint, on the matching parts of the inputs"""
    ob, boxes = geo.out_box, geo.boxes(fam.nin)
    L, U, R = ob[0][d] + lo, ob[0][d] + hi, fam.radius

    def cut(b):
        lb, ub = list(b[0]), list(b[1])
        lb[d], ub[d] = max(lb[d], L - R), min(ub[d], U + R)
        return (lb, ub)
    ob_s = cut(ob)
    boxes_s = [ob_s] + [cut(b) for b in boxes[1:]]
    blb, bub = list(geo.bounds[0]), list(geo.bounds[1])
    blb[d], bub[d] = max(blb[d], L), min(bub[d], U)
    host = [_host_part(f, b) for f, b in zip(ins, boxes_s)]
    take = tuple(slice(L - ob_s[0][d], U - ob_s[0][d]) if a == d else slice(None) for a in range(fam.rank))
    if blb[d] >= bub[d]:
        return host[0][take]                      # no apply point in the range: copy-through of input 0
    out = np.zeros_like(host[0])
    oracle.Module.parse(fam.text(ob_s, (blb, bub), boxes_s)).call("entry", out, *host)
    return out[take]


def _device_part(field, d, lo, hi):
    sl = tuple(slice(lo, hi) if a == d else slice(None) for a in range(field.rank))
    return field.tensor[sl].cpu().numpy()


def check_against_oracle(fam, geo, ins, got, longest_chunk):
    """the direct result against the oracle: the whole field when that is cheap, else the first and last planes,
    both sides of every seam of the longest chunk, and (rank 3) the rows past the last whole row tile of any tile"""
    n0 = geo.shape[0]
    parts = []
    if np.prod(geo.shape) * fam.nacc <= 2.5e8:
        parts.append((0, 0, n0))
    else:
        planes = {0, 1, n0 - 2, n0 - 1}
        for m in range(longest_chunk, n0, longest_chunk):
            planes |= {m - 1, m}
        parts += [(0, p, p + 1) for p in sorted(planes)]
    if fam.rank == 3:
        n1 = geo.shape[1]
        parts.append((1, n1 - 9, n1))               # row-tail trim leaves up to tileJ / 8 <= 8 rows to the direct kernel
    for d, lo, hi in parts:
        want = oracle_part(fam, geo, ins, d, lo, hi)
        have = _device_part(got, d, lo, hi)
        assert bits_equal(have, want), f"{fam.name} {geo.shape} dim {d} [{lo}, {hi}) vs oracle\n" + mismatch_report(have, want)
    return len(parts)


def _sweep_geometry(nh, fam, geo, entry, log):
    torch, capi, apply = nh.torch, nh.capi, nh.apply
    dt = _dtype(nh, fam.elem)
    boxes = geo.boxes(fam.nin)
    ins = [nh.fields.DeviceField.hashed([u - l for l, u in zip(*b)], dt, seed=77 + k, lb=b[0]) for k, b in enumerate(boxes)]
    ref = nh.fields.DeviceField(geo.out_box[0], geo.out_box[1], dt)
    out = nh.fields.DeviceField.empty_like(ref)
    n0 = geo.shape[0]
    tiles = default_tiles(fam.rank)
    assert entry.num_variants == len(tiles), (fam.name, entry.num_variants, len(tiles))

    def launch(f, cfg, region=None):
        apply.apply_builtin(entry, ins, f, geo.bounds, region=region, cfg=cfg)

    def whole(d0_lo, d0_hi):
        return ([d0_lo] + [0] * (fam.rank - 1), [d0_hi] + list(geo.shape[1:]))

    ref.tensor.fill_(float("nan"))
    launch(ref, apply.make_cfg(capi.KERNEL_DIRECT))
    assert _last(nh) == (capi.KERNEL_DIRECT, -1, 0)
    out.tensor.fill_(float("nan"))
    launch(out, apply.make_cfg(capi.KERNEL_DIRECT, flags=capi.FLAG_DIRECT_FLAT))
    assert _last(nh) == (capi.KERNEL_DIRECT, -1, 0)
    assert apply.count_mismatch(out, ref) == 0, f"{fam.name}: flat direct kernel != rows direct kernel"

    def planes_of(tile, lo, hi):
        # the rank-2 tile forms (and every tile of a footprint only the LDS tile kernel holds) treat the field as ONE plane
        jk = fam.rank == 2 and (fam.tile2_only or tiles[tile]["jk"])
        return 1 if jk else hi - lo

    def check(what, want_tile, chunk, planes):
        k, v, c = _last(nh)
        assert k == capi.KERNEL_MARCH and v == want_tile, f"{fam.name} {what}: launched {(k, v, c)}"
        if chunk > 0:
            assert c == min(chunk, planes), f"{fam.name} {what}: chunk {c}, asked {chunk} on {planes} planes"
        else:
            assert 0 < c <= planes, f"{fam.name} {what}: automatic chunk {c} on {planes} planes"
        bad = apply.count_mismatch(out, ref)
        if bad:
            got = out.numpy()
            pytest.fail(f"{fam.name} {geo.shape} {what}: {bad} cells differ from the direct kernel\n" + mismatch_report(got, ref.numpy()))

    # the automatic tile and chunk
    out.tensor.fill_(float("nan"))
    launch(out, apply.make_cfg(capi.KERNEL_MARCH))
    auto = _last(nh)
    assert auto[0] == capi.KERNEL_MARCH, f"{fam.name}: the automatic march launch ran {auto}"
    check("automatic", auto[1], 0, planes_of(auto[1], 0, n0))
    if geo.auto_tile is not None:
        assert auto[1] == geo.auto_tile, f"{fam.name} {geo.shape}: automatic tile {auto[1]}, expected {geo.auto_tile}"

    a, b = fam.radius + 1, n0 - fam.radius - 1
    for t in range(entry.num_variants):
        for chunk in swept_chunks(n0):
            out.tensor.fill_(float("nan"))
            launch(out, apply.make_cfg(capi.KERNEL_MARCH, t, chunk))
            check(f"tile {t} chunk {chunk}", t, chunk, planes_of(t, 0, n0))
        # interior first, then the two edges (lowered_runtime.hpp's halo-exchange split, the slab path)
        out.tensor.fill_(float("nan"))
        for lo, hi in ((a, b), (0, a), (b, n0)):
            launch(out, apply.make_cfg(capi.KERNEL_MARCH, t), region=whole(lo, hi))
            k, v, c = _last(nh)
            assert k == capi.KERNEL_MARCH and v == t and 0 < c <= planes_of(t, lo, hi), (fam.name, t, lo, hi, (k, v, c))
        check(f"tile {t} regions", t, 0, n0)
    longest = max([c for c in swept_chunks(n0) if 0 < c < n0], default=n0)
    parts = check_against_oracle(fam, geo, ins, ref, longest)
    log.append({"family": fam.name, "shape": geo.shape, "tiles": entry.num_variants, "chunks": swept_chunks(n0),
                "auto": auto, "oracle_parts": parts})
    del ins, ref, out
    torch.cuda.empty_cache()
    return auto


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FAMILIES))
def test_sweep_every_tile_and_tuner_chunk(nh, name):
    """every default tile x every tuner chunk length, the automatic choice and the region split of one family: bit for
    bit against the direct kernel on every cell; the direct kernel against the oracle"""
    fam = FAMILIES[name]
    log = []
    for geo in fam.geoms:
        entry = nh.lowering.compile_module(fam.module_text(geo)).geom_entry(fam.function)
        _sweep_geometry(nh, fam, geo, entry, log)
    for rec in log:
        print("SWEEP", json.dumps(rec))


@pytest.mark.gpu
def test_automatic_choice_lands_on_every_default_tile(nh):
    """across the families, the automatic choice lands on each default tile pick_march_variant can pick for them at
    these sizes (tile 6 needs the largest fields: the headline child); tile 5 is the automatic choice only of wide
    footprints the march kernel runs, and every such footprint here runs the plane kernel instead"""
    capi = nh.capi
    seen = {3: set(), 2: set()}
    for fam in FAMILIES.values():
        for geo in fam.geoms:
            entry = nh.lowering.compile_module(fam.module_text(geo)).geom_entry(fam.function)
            dt = _dtype(nh, fam.elem)
            ins = [nh.fields.DeviceField.hashed([u - l for l, u in zip(*b)], dt, seed=1, lb=b[0]) for b in geo.boxes(fam.nin)]
            out = nh.fields.DeviceField(geo.out_box[0], geo.out_box[1], dt)
            nh.apply.apply_builtin(entry, ins, out, geo.bounds, cfg=nh.apply.make_cfg(capi.KERNEL_MARCH))
            k, v, c = _last(nh)
            assert k == capi.KERNEL_MARCH and v == geo.auto_tile, (fam.name, geo.shape, (k, v, c))
            seen[fam.rank].add(v)
            del ins, out
    nh.torch.cuda.empty_cache()
    print("AUTO_TILES", {r: sorted(s) for r, s in seen.items()})
    assert seen[3] >= {0, 1, 2, 3, 4, 7}, seen
    assert seen[2] == set(range(len(default_tiles(2)))), seen


# ---- child processes ---------------------------------------------------------------------------------------------
PRELUDE = f"""
import ctypes as C, json, os, sys
sys.path.insert(0, {str(REPO / 'neptune-pde-solver_amd')!r}); sys.path.insert(0, {str(REPO / 'tests')!r})
sys.path.insert(0, {str(REPO / 'tools')!r})
import numpy as np, torch, helpers
from helpers import oracle, bits_equal, mismatch_report
from neptune_hip import lowering, _capi, apply, fields
lib = _capi.load()
lib.neptune_hip_init(0)
def last():
    c = _capi.LaunchCfg()
    assert lib.neptune_hip_last_launch(C.byref(c)) == 1
    return [c.kernel, c.variant, c.chunk]
"""


def run_child(tmp_path, name, code, timeout, env=None):
    """one fresh interpreter (never exec); a child ended by a signal or the time limit fails the test at once"""
    script = tmp_path / f"{name}.py"
    script.write_text(PRELUDE + code)
    e = dict(os.environ)
    e.pop("NEPTUNE_HIP_TUNE", None)
    e.update({"NEPTUNE_CACHE_DIR": str(tmp_path), "NEPTUNE_HIP_WISDOM": str(tmp_path / "wisdom.txt")})
    e.update(env or {})
    try:
        p = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=timeout, env=e)
    except subprocess.TimeoutExpired as ex:
        pytest.fail(f"{name}: no result within {timeout} s\n{(ex.stdout or '')[-2000:]}")
    if p.returncode < 0:
        pytest.fail(f"{name}: ended by signal {-p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    assert p.returncode == 0, f"{name}: exit {p.returncode}\n{p.stdout[-3000:]}\n{p.stderr[-4000:]}"
    print(p.stdout)
    return p.stdout


def _results(stdout, tag):
    return [json.loads(line.split(tag, 1)[1]) for line in stdout.splitlines() if line.startswith(tag)]


def _prefetch_into(directory, texts):
    """compile module texts into a child's module cache with host threads (nothing is loaded)"""
    from neptune_hip import lowering
    with ThreadPoolExecutor(max_workers=max(1, min(12, len(texts)))) as pool:
        list(pool.map(lambda t: lowering.compile_module(t, cache_directory=directory, load=False), texts))


@pytest.mark.gpu
def test_lowered_headline_on_its_tuned_choice(nh, tmp_path):
    """the module bench.py times (stencil_module("3d7", [1024]*3), the opdef's geometry entry), launched with a free
    choice and default first-use tuning: bit-exact against the direct kernel on every cell and against the oracle on
    the ten planes test_full_size_3d samples; the same for 27-point f32 512^3 and 5-point f64 8192^2"""
    import make_stencil_mlir
    cases = [("3d7", [1024] * 3, 0), ("3d27", [512] * 3, 1), ("2d5", [8192] * 2, 0)]
    _prefetch_into(tmp_path, [make_stencil_mlir.stencil_module(k, s) for k, s, _ in cases])
    code = f"""
import make_stencil_mlir
for kind, shape, code in {cases!r}:
    text = make_stencil_mlir.stencil_module(kind, shape)
    entry = lowering.compile_module(text).geom_entry(make_stencil_mlir.KINDS[kind][2])
    fin = fields.DeviceField.hashed(shape, code, seed=2024)
    f_t = fields.DeviceField.empty_like(fin); f_d = fields.DeviceField.empty_like(fin)
    f_t.tensor.fill_(float("nan")); f_d.tensor.fill_(float("nan"))
    bounds = ([1] * len(shape), [n - 1 for n in shape])
    apply.apply_builtin(entry, [fin], f_t, bounds)              # free choice: first-use tuning, wisdom written
    tuned = last()
    apply.apply_builtin(entry, [fin], f_d, bounds, cfg=apply.make_cfg(_capi.KERNEL_DIRECT))
    torch.cuda.synchronize()
    bad = apply.count_mismatch(f_t, f_d)
    ok = 0
    if len(shape) == 3:
        n0 = shape[0]
        planes = [0, 1, 2, n0 // 2 - 1, n0 // 2, n0 - 2, n0 - 1, 127, 128, 129]
        for i in planes:
            got = f_t.planes(i, i + 1)[0]
            if i in (0, n0 - 1):
                want = fin.planes(i, i + 1)[0]
            else:
                want = helpers.oracle_entry(kind, fin.planes(i - 1, i + 2))[1]
            if bits_equal(got, want):
                ok += 1
            else:
                print(f"plane {{i}}:", mismatch_report(got, want))
    else:
        planes = [None]
        got, want = f_t.numpy(), helpers.oracle_entry(kind, fin.numpy())
        ok = int(bits_equal(got, want))
    stats = (C.c_int64 * 3)(); lib.neptune_hip_tune_stats(stats)
    peak = torch.cuda.max_memory_allocated()
    print("HEADLINE" + json.dumps({{"kind": kind, "shape": shape, "tuned": tuned, "mismatch": bad, "oracle_ok": ok,
                                   "oracle_parts": len(planes), "measured": stats[0], "peak_gib": round(peak / 2**30, 2)}}), flush=True)
    del fin, f_t, f_d
    torch.cuda.empty_cache()
"""
    res = _results(run_child(tmp_path, "headline", code, timeout=900), "HEADLINE")
    assert [r["kind"] for r in res] == [c[0] for c in cases], res
    for r in res:
        assert r["mismatch"] == 0 and r["oracle_ok"] == r["oracle_parts"], r
        assert r["tuned"][0] == nh.capi.KERNEL_MARCH and r["tuned"][2] > 0, r
    assert res[-1]["measured"] == 3, res                       # each of the three tuned itself on first use
    assert (tmp_path / "wisdom.txt").read_text().count("\n") == 3


def _family_setup_code(fam, geo):
    """child code that builds (text, entry, ins, bounds, region-free launch helpers) for one family geometry"""
    return f"""
fam_text = {fam.module_text(geo)!r}
entry = lowering.compile_module(fam_text).geom_entry({fam.function!r})
boxes = {geo.boxes(fam.nin)!r}
dt = {_dtype_code(fam.elem)}
ins = [fields.DeviceField.hashed([u - l for l, u in zip(*b)], dt, seed=77 + k, lb=b[0]) for k, b in enumerate(boxes)]
bounds = {geo.bounds!r}
ref = fields.DeviceField(boxes[0][0], boxes[0][1], dt); ref.tensor.fill_(float("nan"))
apply.apply_builtin(entry, ins, ref, bounds, cfg=apply.make_cfg(_capi.KERNEL_DIRECT))
def run(cfg):
    out = fields.DeviceField.empty_like(ref); out.tensor.fill_(float("nan"))
    apply.apply_builtin(entry, ins, out, bounds, cfg=cfg)
    ran = last()
    bad = apply.count_mismatch(out, ref)
    return ran, bad
"""


def _dtype_code(elem):
    return "_capi.F64" if elem == "f64" else "_capi.F32"


@pytest.mark.gpu
def test_tuners_pick_only_what_the_sweep_ran(nh, tmp_path):
    """NEPTUNE_HIP_TUNE=1: for each family, the first-use tuner's free choice and neptune_hip_autotune_fn's pick are
    bit-exact against the direct kernel, and each is the automatic choice or a (tile, chunk as launched) the sweep runs"""
    geos = [(fam, fam.geoms[0]) for fam in FAMILIES.values()]
    _prefetch_into(tmp_path, [fam.module_text(g) for fam, g in geos])
    code = ""
    for fam, geo in geos:
        code += _family_setup_code(fam, geo) + f"""
free, free_bad = run(None)
best, ms = apply.autotune_builtin(entry, ins, fields.DeviceField.empty_like(ref), bounds)
picked = [best.kernel, best.variant, best.chunk]
ran, bad = run(best)
print("TUNED" + json.dumps({{"family": {fam.name!r}, "free": free, "free_bad": free_bad, "plan_pick": picked, "plan_ran": ran,
                            "plan_bad": bad}}), flush=True)
del ins, ref
torch.cuda.empty_cache()
"""
    out = run_child(tmp_path, "tuners", code, timeout=900, env={"NEPTUNE_HIP_TUNE": "1"})
    res = {r["family"]: r for r in _results(out, "TUNED")}
    assert list(res) == [fam.name for fam, _ in geos], out[-2000:]
    # the first-use tuner's choices, in the order the families ran (wisdom.hip: "<key>\t<kernel> <variant> <chunk> ...")
    lines = (tmp_path / "wisdom.txt").read_text().splitlines()
    assert len(lines) == len(geos), lines
    for (fam, geo), line in zip(geos, lines):
        r = res[fam.name]
        r["free_pick"] = [int(x) for x in line.split("\t")[1].split()[:3]]
        assert r["free_bad"] == 0 and r["plan_bad"] == 0, r
        assert r["free"][0] == nh.capi.KERNEL_MARCH and r["plan_ran"][0] == nh.capi.KERNEL_MARCH, r
        for what in ("free_pick", "plan_pick"):
            k, v, c = r[what]
            assert (k, v, c) == (nh.capi.KERNEL_AUTO, -1, 0) or (
                k == nh.capi.KERNEL_MARCH and 0 <= v < len(default_tiles(fam.rank)) and (c == 0 or min(c, geo.shape[0]) in swept_chunks(geo.shape[0]))), \
                f"{fam.name}: the {what} {(k, v, c)} is outside what the sweep runs"
        print("TUNER_PICKS", fam.name, "first use", r["free_pick"], "ran", r["free"], "plan time", r["plan_pick"], "ran", r["plan_ran"])


# ---- the launch-choice key and aliased outputs -------------------------------------------------------------------
def _key_case():
    """one lowered apply whose input 1 (read with a 7-point star) sits, in call A, in a box that contains the result's
    (march kernel) and, in call B, in a box of the same extents shifted along K that does not (direct kernel): the same
    result geometry, the same alignment, bounds whose accesses stay inside both"""
    from test_ownbox_gpu import module_text
    shape = (12, 20, 256)
    ob = _box(shape)
    bounds = ([1, 1, 2], [11, 19, 255])
    acc = [(0, (0, 0, 0)), (1, (0, 0, 0))] + [(1, o) for o in _star(3, 1)]
    in_a = ([-1, -1, -1], [13, 21, 257])
    in_b = ([-1, -1, 1], [13, 21, 259])
    return {g: (module_text("f64", ob, bounds, [ob, b], acc), [ob, b]) for g, b in (("A", in_a), ("B", in_b))}, bounds


KEY_CHILD = """
from neptune_hip.fields import current_stream_ptr
cases, bounds = {cases!r}, {bounds!r}
entry = lowering.compile_module(cases["A"][0]).geom_entry("resid")
for g in {order!r}:
    text, boxes = cases[g]
    ins = [fields.DeviceField.hashed([u - l for l, u in zip(*b)], _capi.F64, seed=5 + k, lb=b[0]) for k, b in enumerate(boxes)]
    out = fields.DeviceField(boxes[0][0], boxes[0][1], _capi.F64)
    out.tensor.fill_(float("nan"))
    rc = entry(apply.geom_for(ins, out, bounds), apply._in_array(ins), out.ptr, current_stream_ptr(), None)   # free choice
    ran = last() if rc == 0 else None
    torch.cuda.synchronize()
    exact = False
    if rc == 0:
        want = np.zeros(out.shape)
        oracle.Module.parse(text).call("entry", want, *[f.numpy() for f in ins])
        exact = bits_equal(out.numpy(), want)
    print("KEY" + json.dumps({{"geometry": g, "rc": rc, "ran": ran, "exact": exact}}), flush=True)
"""


@pytest.mark.gpu
def test_launch_choice_key_tells_input_boxes_apart(nh, tmp_path):
    """a choice remembered for geometry A (input 1 in a box containing the result's: a march tile) is not handed to
    geometry B (input 1 in a box that does not: direct kernel only) of the same result geometry -- not from the wisdom
    file in a later process, not from the in-process table after A ran"""
    cases, bounds = _key_case()
    _prefetch_into(tmp_path, [cases["A"][0]])
    tune = {"NEPTUNE_HIP_TUNE": "1"}

    def child(name, order):
        return {r["geometry"]: r for r in _results(run_child(tmp_path, name, KEY_CHILD.format(cases=cases, bounds=bounds, order=order),
                                                             timeout=300, env=tune), "KEY")}
    a = child("key_a", ["A"])["A"]
    assert a["rc"] == 0 and a["exact"] and a["ran"][0] == nh.capi.KERNEL_MARCH, a
    wisdom = tmp_path / "wisdom.txt"
    lines = wisdom.read_text().splitlines()
    assert len(lines) == 1, lines
    # the same key, now holding a forced march tile and chunk (the last line of a key wins): A's choice is that tile
    forced = (nh.capi.KERNEL_MARCH, 3, 4)
    with open(wisdom, "a") as f:
        f.write(lines[0].split("\t")[0] + "\t%d %d %d 0 0.001\n" % forced)
    b = child("key_b", ["B"])["B"]
    assert b["rc"] == 0 and b["exact"] and b["ran"][0] == nh.capi.KERNEL_DIRECT, b
    ab = child("key_ab", ["A", "B"])
    assert ab["A"]["rc"] == 0 and ab["A"]["exact"] and tuple(ab["A"]["ran"]) == forced, ab
    assert ab["B"]["rc"] == 0 and ab["B"]["exact"] and ab["B"]["ran"][0] == nh.capi.KERNEL_DIRECT, ab


@pytest.mark.gpu
def test_geometry_entries_refuse_aliased_output(nh):
    """<tag>__geom and __geom2 return NEPTUNE_HIP_EINVAL and launch nothing when the output is an input or overlaps
    part of it, as neptune_hip_apply_builtin does"""
    import make_stencil_mlir
    torch, capi = nh.torch, nh.capi
    from neptune_hip.fields import current_stream_ptr
    shape = (12, 20, 256)
    entry = nh.lowering.compile_module(make_stencil_mlir.stencil_module("3d7", list(shape))).geom_entry("lap3d")
    assert entry.fn2 is not None
    count = int(np.prod(shape))
    base = torch.empty(2 * count, dtype=torch.float64, device="cuda")
    base.copy_(torch.from_numpy(helpers.hash_field((2 * count,), np.float64, seed=3)))
    lb, ub = (0, 0, 0), shape
    fin = nh.fields.DeviceField(lb, ub, capi.F64, base[:count].view(shape))
    partial = nh.fields.DeviceField(lb, ub, capi.F64, base[count // 2:count // 2 + count].view(shape))
    bounds = ([1, 1, 1], [n - 1 for n in shape])
    for name, fn in (("__geom", entry.fn), ("__geom2", entry.fn2)):
        for out in (fin, partial):
            before = base.clone()
            g = nh.apply.geom_for([fin], out, bounds)
            rc = fn(C.byref(g), nh.apply._in_array([fin]), out.ptr, current_stream_ptr(), None)
            torch.cuda.synchronize()
            assert rc == capi.EINVAL, f"{name}: aliased output (offset {out.ptr - fin.ptr} B) returned {rc}"
            assert torch.equal(base.view(torch.int64), before.view(torch.int64)), f"{name}: the refused launch wrote"
    # distinct buffers still run (and __geom2 qualifies for this geometry)
    out = nh.fields.DeviceField(lb, ub, capi.F64, base[count:].view(shape))
    g = nh.apply.geom_for([fin], out, bounds)
    assert entry.fn(C.byref(g), nh.apply._in_array([fin]), out.ptr, current_stream_ptr(), None) == 0
    assert entry.fn2(C.byref(g), nh.apply._in_array([fin]), out.ptr, current_stream_ptr(), None) == 0
    torch.cuda.synchronize()
