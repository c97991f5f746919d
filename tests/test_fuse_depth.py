"""fuse_depth_maps (csrc/depth_fuse.hip): multi-view depth-map fusion — consistency filter, ownership, cloud.

tests/fuse_depth_ref.py restates the three passes in numpy fp64 by the plain chain of the definition; tests/depth_scenes.py renders the
scenes and asserts that no decision of the restatement lies within 1e-6 of its threshold.  The kernel takes the same decisions from
pair constants in fp64, which differ from the plain chain by rounding order only (1e-12 px at the world offset of 1e4), so valid, views,
num_views, view, pixel, point_views and counts are compared for EQUALITY.  depth and points are compared within ONE fp32 ulp of the
restatement's fp64 value rounded to fp32: one ulp allows for a final rounding that falls the other way.  The points are compared with
the restatement's formula applied to the fused depth the device stored (itself checked), since they are defined from that fp32 value.

Seeds: every scene uses seed 0; all of them are clean at 1e-6 (of the scenes with V = 5, seeds 1 and 2 are not: a relative depth error
8.9e-7 and 8.5e-7 from the threshold)."""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import depth_scenes as DS
from tests import fuse_depth_ref as FR
from tests.helpers import kernel_resources

DEV = "cuda:0"
PIXELS_PER_BLOCK = 1024                                            # csrc/depth_fuse.hip
PER_PIXEL = ("valid", "views", "num_views")
CLOUD = ("view", "pixel", "point_views")


# ------------------------------------------------------------------------------------------------------------------ CPU
def test_restatement_keeps_what_another_view_sees_and_drops_wrong_depths():
    """Noise-free maps.  Pixel (r, i, j) is seen unoccluded by view s when its point projects in front of s, the ray of s through that
    projection meets the same surface at the point's depth, and the four taps around it lie inside the map on that surface: then s must
    be consistent, and the pixel valid.  With 5 % of the depths scaled by 1.3 (and 5 % holes) no scaled pixel of this scene (V = 3, seed
    0, 108 scaled pixels) is valid, and no hole.  That is what the filter is for, not a theorem: a scaled pixel survives when another
    view's sample on its ray happens to be wrong by the same factor, or is a bilinear blend across the rectangle's edge that passes
    through the wrong depth (seeds 1 and 4 have 2 and 1 such pixels at V = 3; V = 5 at seed 0 has 4)."""
    V = 3
    sc = DS.fuse_scene(V, 0, perturb=False)
    ref, K, R, t = sc["ref"], sc["K"], sc["R"], sc["t"]
    checked = 0
    for r in range(V):
        H, W = sc["shapes"][r]
        ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        u, v, d = (jj + 0.5).ravel(), (ii + 0.5).ravel(), sc["clean"][r].ravel()
        X = FR.lift(u, v, d, np.linalg.inv(K[r]), R[r], t[r])
        seen_by_any = np.zeros(H * W, bool)
        for s in range(V):
            if s == r:
                continue
            Hs, Ws = sc["shapes"][s]
            q = FR.project(X, K[s], R[s], t[s])
            us, vs = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
            x0, y0 = np.floor(us - 0.5).astype(int), np.floor(vs - 0.5).astype(int)
            inside = (q[:, 2] > 0) & (x0 >= 0) & (x0 + 1 < Ws) & (y0 >= 0) & (y0 + 1 < Hs) & (d > 0)
            ds, ss = DS.render(K[s], R[s], t[s], None, pix=np.stack([us, vs], -1))
            same = inside & (ss == sc["surface"][r].ravel()) & (np.abs(ds - q[:, 2]) < 1e-9 * q[:, 2])
            x0, y0 = np.clip(x0, 0, Ws - 2), np.clip(y0, 0, Hs - 2)
            for dy in (0, 1):
                for dx in (0, 1):
                    same &= sc["surface"][s][y0 + dy, x0 + dx] == sc["surface"][r].ravel()
            assert ref["consistent"][r][s].ravel()[same].all(), (r, s)
            seen_by_any |= same
            checked += int(same.sum())
        assert ref["valid"][r].ravel()[seen_by_any].all()
    assert checked > 1500                                            # of 3 * 2 * 768 pairs of pixel and view
    wr = DS.fuse_scene(V, 0, noise=False)
    n_wrong = sum(int(w.sum()) for w in wr["wrong"])
    assert n_wrong > 100
    for v in range(V):
        assert not (wr["ref"]["valid"][v] & wr["wrong"][v]).any()
        assert not wr["ref"]["valid"][v][wr["hole"][v]].any()


@pytest.mark.parametrize("V", [2, 3, 5])
def test_every_chain_of_duplicates_ends_in_an_emitted_pixel(V):
    ref = DS.fuse_scene(V, 0)["ref"]
    assert ref["counts"][1] == ref["counts"][0] + ref["counts"][2] and ref["counts"][2] > 0
    assert not ref["dup"][0].any()                                   # the lowest view owns everything it has
    ends = 0
    for r in range(V):
        assert not (ref["dup"][r] & ~ref["valid"][r]).any()
        for i, j in zip(*np.nonzero(ref["valid"][r])):
            at = (r, i, j)
            while not ref["emit"][at[0]][at[1], at[2]]:
                nxt = tuple(int(x) for x in ref["owner"][at[0]][at[1], at[2]])
                assert 0 <= nxt[0] < at[0] and ref["valid"][nxt[0]][nxt[1], nxt[2]]      # strictly lower, and valid itself
                at = nxt
            ends += 1
    assert ends == ref["counts"][1]                                  # no valid pixel is lost


def _host_tables(side=8):
    buf = (ctypes.c_double * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    ptrs = (ctypes.c_void_p * 33)(*[ctypes.addressof(buf)] * 33)
    dims = (ctypes.c_int * 66)(*[side] * 66)
    return buf, a, ptrs, dims


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    buf, a, ptrs, dims = _host_tables()
    pt, dm = ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(dims, ctypes.c_void_p)

    def call(depths=pt, dims=dm, K=a, R=a, t=a, V=2, reproj=1.0, rel=0.01, min_views=2, T=16, depth=a, valid=a, views=a, num=a, points=a,
             view=a, pixel=a, pviews=a, counts=a, ws=a, ws_bytes=1 << 20):
        return lib.roma_depth_fuse(depths, dims, K, R, t, V, reproj, rel, min_views, T, depth, valid, views, num, points, view, pixel, pviews,
                                   counts, ws, ws_bytes, None)

    for kw in ("depths", "dims", "K", "R", "t", "depth", "valid", "views", "num", "points", "view", "pixel", "pviews", "counts", "ws"):
        assert call(**{kw: None}) == _lib.ROMA_E_ARG and b"roma_depth_fuse: null pointer" in lib.roma_last_error(), kw
    null_map = (ctypes.c_void_p * 2)(ctypes.addressof(buf), None)
    assert call(depths=ctypes.cast(null_map, ctypes.c_void_p)) == _lib.ROMA_E_ARG and b"depth map of view 1" in lib.roma_last_error()
    for V in (1, 33):
        assert call(V=V) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error()
        assert lib.roma_depth_fuse_workspace(V, 1000, None) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error()
    big = (ctypes.c_int * 4)(8, 8, 32769, 8)
    assert call(dims=ctypes.cast(big, ctypes.c_void_p)) == _lib.ROMA_E_SHAPE and b"bad shape map 1 is 32769x8" in lib.roma_last_error()
    big = (ctypes.c_int * 4)(8, 0, 8, 8)
    assert call(dims=ctypes.cast(big, ctypes.c_void_p)) == _lib.ROMA_E_SHAPE and b"bad shape" in lib.roma_last_error()
    full = (ctypes.c_int * 6)(32768, 32768, 32768, 32768, 1, 1)         # 2^31 pixels after the second map: the total does not fit an int
    assert call(dims=ctypes.cast(full, ctypes.c_void_p), V=3) == _lib.ROMA_E_SHAPE and b"2^31 - 1 pixels" in lib.roma_last_error()
    for total in (1, 1 << 31):
        assert lib.roma_depth_fuse_workspace(2, total, None) == _lib.ROMA_E_SHAPE and b"total_pixels" in lib.roma_last_error()
    for kw in (dict(reproj=0.0), dict(rel=-1.0), dict(reproj=float("nan")), dict(rel=float("nan"))):
        assert call(**kw) == _lib.ROMA_E_ARG and b"must be positive" in lib.roma_last_error()
    for mv in (1, 3):
        assert call(min_views=mv) == _lib.ROMA_E_ARG and b"min_views" in lib.roma_last_error()
    assert call(T=0) == _lib.ROMA_E_ARG and b"max_points" in lib.roma_last_error()
    assert call(ws_bytes=100) == _lib.ROMA_E_ARG and b"workspace of 100 bytes" in lib.roma_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(buf) + 8)
    assert call(ws=odd) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()
    # the workspace: one flag per pixel and 12 bytes per block of 1024 pixels, at most total / 1024 + V blocks, each rounded up to 256
    sizes = (ctypes.c_long * 2)()
    need = lib.roma_depth_fuse_workspace(32, 32 * 864 * 864, ctypes.cast(sizes, ctypes.c_void_p))
    assert list(sizes) == [32 * 864 * 864, -(-12 * (32 * 864 * 864 // 1024 + 32) // 256) * 256] and need == sum(sizes)


def test_wrapper_validates_before_it_looks_at_a_tensor():
    from roma_amd import geometry
    d = [torch.ones(4, 6), torch.ones(4, 6)]
    R, t, K = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.eye(3)
    ok = dict(max_points=10)
    for kw in (dict(max_reproj_error=0.0), dict(max_reproj_error=float("nan")), dict(max_depth_error=-0.1), dict(max_depth_error=float("inf")),
               dict(min_views=1), dict(min_views=3), dict(max_points=0), dict(max_points=1 << 31), dict(max_points=None),
               dict(sizes=[(4, 6)]), dict(sizes=[(4, 6), (0, 6)]), dict(sizes=7)):
        with pytest.raises(ValueError):
            geometry.fuse_depth_maps(d, R, t, K, **{**ok, **kw})
    with pytest.raises(TypeError):
        geometry.fuse_depth_maps(d, R, t, K)                         # max_points is required
    for bad in (dict(R=torch.eye(3).expand(3, 3, 3)), dict(t=torch.zeros(3, 3)), dict(K=torch.eye(3).expand(3, 3, 3)), dict(K=torch.eye(4))):
        args = {**dict(R=R, t=t, K=K), **bad}
        with pytest.raises(ValueError, match="expected"):
            geometry.fuse_depth_maps(d, args["R"], args["t"], args["K"], **ok)
    for maps in (d[:1], [torch.ones(4, 6)] * 33, [torch.ones(4, 6), torch.ones(6)], torch.ones(2, 4, 6, 1), "maps", [d[0], 3.0]):
        with pytest.raises(ValueError):
            geometry.fuse_depth_maps(maps, R, t, K, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.fuse_depth_maps(d, R, t, K, **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.fuse_depth_maps(torch.ones(2, 4, 6), R, t, K, **ok)


def test_depth_fuse_kernels_resource_report():
    """The compiler's resource report of csrc/depth_fuse.hip (the table of DESIGN.md §3.4): five kernels, none with scratch, static LDS
    only and far within the 160 KiB of a compute unit."""
    kernels = kernel_resources("depth_fuse.hip")
    names = ("consistency", "ownership", "scan", "clear", "cloud")
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch | occupancy |")
    for n in names:
        (k,) = [v for name, v in kernels.items() if f"fuse_{n}_kernel" in name]
        print(f"| `fuse_{n}_kernel` | {k['VGPRs']} | {k['TotalSGPRs']} | {k['LDS Size']} | {k['ScratchSize']} | {k['Occupancy']} |")
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
        assert k["LDS Size"] <= 160 * 1024
    assert len(kernels) == len(names), sorted(kernels)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _run(depths, R, t, K, stacked=False, **kw):
    from roma_amd import geometry
    maps = _dev(np.stack(depths)) if stacked else [_dev(d) for d in depths]
    out = geometry.fuse_depth_maps(maps, _dev(R), _dev(t), _dev(K), **kw)
    torch.cuda.synchronize()
    assert torch.is_tensor(out.depth) == stacked
    got = {k: [a.cpu().numpy() for a in getattr(out, k)] for k in ("depth",) + PER_PIXEL}
    got.update({k: getattr(out, k).cpu().numpy() for k in ("points", "counts") + CLOUD})
    return got


def _ulp_close(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    with np.errstate(all="ignore"):
        ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got))).astype(np.float64)
        return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp


def _compare(got, ref, depths, R, t, K, sizes, T):
    """got: _run's result at max_points = T; ref: the restatement's with every emitted pixel in its cloud"""
    V = len(depths)
    assert got["counts"].dtype == np.int32 and np.array_equal(got["counts"], ref["counts"]) and got["counts"][3] == 0
    for v in range(V):
        for name in PER_PIXEL:
            assert got[name][v].dtype == ref[name][v].dtype and np.array_equal(got[name][v], ref[name][v]), (name, v)
        assert got["depth"][v].dtype == np.float32 and _ulp_close(got["depth"][v], ref["depth"][v]).all(), v
        assert (got["depth"][v][~ref["valid"][v]] == 0).all()
    k = min(int(ref["counts"][0]), T)
    for name in CLOUD:
        assert got[name].shape == (T,) and got[name].dtype == ref[name].dtype and np.array_equal(got[name][:k], ref[name][:k]), name
    assert (got["pixel"][k:] == -1).all() and not got["view"][k:].any() and not got["point_views"][k:].any() and not got["points"][k:].any()
    # the points: the definition applied to the fused depth the device stored
    Kmap = FR.scaled_intrinsics(K, [d.shape for d in depths], sizes)
    want = np.zeros((k, 3))
    for v in range(V):
        rows = np.flatnonzero(ref["view"][:k] == v)
        n = ref["pixel"][rows]
        W = depths[v].shape[1]
        want[rows] = FR.lift(n % W + 0.5, n // W + 0.5, np.ones(len(n)), FR.inverse_k(Kmap[v]), np.eye(3), np.zeros(3)) \
            * got["depth"][v].ravel()[n].astype(np.float64)[:, None]
        want[rows] = (want[rows] - np.asarray(t, np.float64)[v]) @ np.asarray(R, np.float64)[v]
    assert got["points"].shape == (T, 3) and got["points"].dtype == np.float32
    with np.errstate(all="ignore"):
        assert _ulp_close(got["points"][:k], want.astype(np.float32)).all()
    assert _ulp_close(got["points"][:k], ref["points"][:k]).mean() > 0.99      # and the restatement's own cloud, up to a flipped depth


def _check_scene(sc, T=None, stacked=False, **kw):
    T = int(sc["ref"]["counts"][0]) + 7 if T is None else T
    got = _run(sc["depths"], sc["R"], sc["t"], sc["K"], stacked=stacked, sizes=sc["sizes"], max_points=T, **kw)
    _compare(got, sc["ref"], sc["depths"], sc["R"], sc["t"], sc["K"], sc["sizes"], T)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("V", [2, 3, 5])
def test_matches_the_restatement(V):
    sc = DS.fuse_scene(V, 0)
    got = _check_scene(sc, stacked=(V == 3))
    assert got["counts"][0] > 400 and got["counts"][2] > 200


@pytest.mark.gpu
def test_three_shapes_and_image_sizes_that_differ_from_the_maps():
    """K refers to images of 2x, 2x and (3x, 2x) the maps: the wrapper's scaling of K, per axis, is pinned."""
    sc = DS.fuse_scene(3, 0, shapes=((24, 32), (29, 31), (17, 40)), images=((48, 64), (58, 62), (51, 80)))
    got = _check_scene(sc)
    assert got["counts"][0] > 500 and all(v.mean() > 0.3 for v in sc["ref"]["valid"])


@pytest.mark.gpu
def test_thirty_two_views_use_bit_31():
    sc = DS.fuse_scene(32, 0, shapes=((8, 12),))
    got = _check_scene(sc)
    assert (got["views"][31] < 0).any() and (got["views"][0] < 0).any() and got["num_views"][0].max() > 16


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(31, 33), (32, 32), (25, 41), (45, 50)])
def test_block_edges(shape):
    """1023, 1024 and 1025 pixels — one below, equal to and one above the pixels of a block — and 2250, which spans three blocks"""
    assert shape[0] * shape[1] in (PIXELS_PER_BLOCK - 1, PIXELS_PER_BLOCK, PIXELS_PER_BLOCK + 1, 2250)
    sc = DS.fuse_scene(2, 0, shapes=(shape,))
    got = _check_scene(sc)
    assert got["counts"][0] > shape[0] * shape[1] // 2


@pytest.mark.gpu
def test_blocks_beyond_the_first_pass_of_the_scan():
    """Two maps of 740 x 730: 528 blocks each, 1056 in all, 32 more than the scan kernel's 1024 threads take in one pass, so the ranks
    of the pixels that view 1 emits from its last 45 rows need the carry of the first pass.  At 1.5 million decisions the scene cannot
    keep DS.MARGIN; every decision lies 1e-9 or more from its threshold, four orders above the fp64 rounding of the device's and the
    restatement's expressions (below 1e-13 of quantities of order 1), so the restatement decides each one as the device does."""
    shape = (740, 730)
    sc = DS.fuse_scene(2, 1, shapes=(shape,), check=False)
    assert all(len(m) == 0 or m.min() >= 1e-9 for m in sc["ref"]["margins"].values())
    per_view = -(-shape[0] * shape[1] // PIXELS_PER_BLOCK)
    assert 2 * per_view == 1056
    got = _check_scene(sc)
    k = int(got["counts"][0])
    block = got["view"][:k].astype(np.int64) * per_view + got["pixel"][:k] // PIXELS_PER_BLOCK
    assert (np.diff(block) >= 0).all() and (block >= 1024).sum() > 1000 and (block < 1024).sum() > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("delta", [-300, -1, 0, 1])
def test_max_points_below_equal_and_above(delta):
    sc = DS.fuse_scene(3, 0)
    _check_scene(sc, T=int(sc["ref"]["counts"][0]) + delta)


@pytest.mark.gpu
def test_holes_of_every_kind():
    """NaN, +inf, -inf, negative and zero depths are holes: never a reference pixel, never blended into a sample"""
    sc = DS.fuse_scene(3, 0)
    depths = [d.copy() for d in sc["depths"]]
    rng = np.random.default_rng(17)
    for d in depths:
        for bad in (np.nan, np.inf, -np.inf, -3.0, 0.0, -0.0):
            d.ravel()[rng.choice(d.size, 12, replace=False)] = bad
    ref = FR.fuse_depth_ref(depths, sc["R"], sc["t"], sc["K"])
    assert all(m.min() >= DS.MARGIN for m in ref["margins"].values())
    T = int(ref["counts"][0]) + 5
    got = _run(depths, sc["R"], sc["t"], sc["K"], max_points=T)
    _compare(got, ref, depths, sc["R"], sc["t"], sc["K"], None, T)
    for v in range(3):
        holes = ~FR.is_depth(depths[v])
        assert holes.sum() > 60 and not got["views"][v][holes].any() and not got["valid"][v][holes].any()
        assert np.isfinite(got["depth"][v]).all()
    assert np.isfinite(got["points"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["singular_k", "nan_t", "lower_k"])
def test_an_unusable_view_in_the_middle(how):
    sc = DS.fuse_scene(4, 0)
    K, t = sc["K"].copy(), sc["t"].copy()
    if how == "singular_k":
        K[1, 0, 0] = 0.0
    elif how == "lower_k":
        K[1, 1, 0] = 1e-3
    else:
        t[1, 2] = np.nan
    ref = FR.fuse_depth_ref(sc["depths"], sc["R"], t, K)
    assert all(m.min() >= DS.MARGIN for m in ref["margins"].values())
    T = int(ref["counts"][0]) + 5
    got = _run(sc["depths"], sc["R"], t, K, max_points=T)
    _compare(got, ref, sc["depths"], sc["R"], t, K, None, T)
    assert not got["views"][1].any() and not got["valid"][1].any() and not any(((got["views"][v] >> 1) & 1).any() for v in (0, 2, 3))
    assert got["counts"][0] > 500 and (got["view"] != 1).all()


@pytest.mark.gpu
def test_projections_at_1e30_and_behind_the_camera():
    """View 2 stands 1e30 to the side (the others' pixels project to coordinates of 1e30 px in it), view 3 looks the other way (everything
    is behind it), view 4 stands 1e30 in front (everything is behind it; its own pixels project to a vanishing point INSIDE the other
    maps, are sampled there and come back behind it): none agrees with anything, views 0 and 1 agree as if they were alone."""
    sc = DS.fuse_scene(5, 0)
    R, t = sc["R"].copy(), sc["t"].copy()
    t[2] = [1e30, -2e30, 3e29]
    R[3] = np.diag([-1.0, 1.0, -1.0]) @ R[3]
    t[4] = [1e29, -2e29, -1e30]
    ref = FR.fuse_depth_ref(sc["depths"], R, t, sc["K"])
    two = FR.fuse_depth_ref(sc["depths"][:2], R[:2], t[:2], sc["K"][:2])
    for v in (0, 1):
        assert np.array_equal(ref["views"][v], two["views"][v])
    T = int(ref["counts"][0]) + 5
    got = _run(sc["depths"], R, t, sc["K"], max_points=T)
    assert np.isfinite(got["points"]).all()
    _compare(got, ref, sc["depths"], R, t, sc["K"], None, T)
    for v in (2, 3, 4):
        assert not got["valid"][v].any() and set(np.unique(got["views"][v])) <= {0, 1 << v}


@pytest.mark.gpu
def test_min_views_three():
    sc = DS.fuse_scene(5, 0, min_views=3)
    got = _check_scene(sc, min_views=3)
    assert 300 < got["counts"][1] < DS.fuse_scene(5, 0)["ref"]["counts"][1]


@pytest.mark.gpu
def test_world_offset_changes_nothing_but_the_points():
    near, far = DS.fuse_scene(3, 0), DS.fuse_scene(3, 0, offset=True)
    got = _check_scene(far)
    for v in range(3):
        for name in PER_PIXEL:
            assert np.array_equal(got[name][v], near["ref"][name][v])
        assert _ulp_close(got["depth"][v], near["ref"]["depth"][v]).all()
    k = int(near["ref"]["counts"][0])
    assert np.array_equal(got["counts"], near["ref"]["counts"])
    for name in CLOUD:
        assert np.array_equal(got[name][:k], near["ref"][name])
    assert np.abs(got["points"][:k] - DS.WORLD_OFFSET - near["ref"]["points64"]).max() < 2e-3      # fp32 at 2e4: ulp 2e-3


@pytest.mark.gpu
def test_run_to_run_and_graph_replay_are_bit_identical():
    from roma_amd import geometry
    sc = DS.fuse_scene(5, 0)
    maps, R, t, K = [_dev(d) for d in sc["depths"]], _dev(sc["R"]), _dev(sc["t"]), _dev(sc["K"])
    T = int(sc["ref"]["counts"][0]) - 50

    def call():
        f = geometry.fuse_depth_maps(maps, R, t, K, max_points=T)
        return tuple(f.depth) + tuple(f.valid) + tuple(f.views) + tuple(f.num_views) + (f.points, f.view, f.pixel, f.point_views, f.counts)

    def same(a, b):
        return all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))

    first, second = call(), call()
    assert same(first, second) and int(first[-1][0]) == T + 50
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert same(out, first)


@pytest.mark.gpu
def test_chain_half_resolution_maps_with_full_size_intrinsics():
    """Three 24 x 32 maps of one scene (0.3 % noise, 5 % of the depths scaled by 1.3, 5 % holes) passed with the K of the 48 x 64 images
    and sizes = (48, 64), default thresholds.  The median distance of the fused cloud to the analytic surface must be below that of the
    unfused, unfiltered union of the lifted maps, and no emitted point may come from a scaled pixel (the first test says when one can).
    Measured on an MI355X: 0.0072 for the 997 fused points against 0.0155 for the union of 2 205 pixels; no point from a scaled pixel."""
    V = 3
    sc = DS.fuse_scene(V, 0, images=((48, 64),))
    got = _check_scene(sc)
    k = int(got["counts"][0])
    Kmap = FR.scaled_intrinsics(sc["K"], sc["shapes"], sc["sizes"])
    union = []
    for v in range(V):
        H, W = sc["shapes"][v]
        ii, jj = np.nonzero(sc["depths"][v] > 0)
        union.append(FR.lift(jj + 0.5, ii + 0.5, sc["depths"][v][ii, jj].astype(np.float64), np.linalg.inv(Kmap[v]), sc["R"][v], sc["t"][v]))
    union = np.concatenate(union)
    fused, plain = np.median(DS.surface_distance(got["points"][:k].astype(np.float64))), np.median(DS.surface_distance(union))
    print(f"chain: median distance to the surface {fused:.4f} fused ({k} points) against {plain:.4f} for the union of {len(union)} pixels")
    assert k > 500 and fused < plain
    for v in range(V):
        px = got["pixel"][:k][got["view"][:k] == v]
        assert not sc["wrong"][v].ravel()[px].any()
