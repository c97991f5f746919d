"""render_points (csrc/render_points.hip): the z-buffered point splat into V posed views and the per-point visibility.

tests/render_points_ref.py restates the definition in numpy fp64 by the plain chain; tests/render_scenes.py builds the scenes and asserts
that no decision of the restatement lies within 1e-6 of its threshold.  The kernel projects through P_v = K_v [R_v | t_v] with fused
multiply-adds, which differs from the plain chain by fp64 rounding order only, so index, visible, num_views and counts are compared
for EQUALITY and depth within ONE fp32 ulp (a final rounding that falls the other way).

Seeds 0, 1 and 2 at 24 x 32 with Vs = 3: the smallest border distance is 7.7e-5 to 2.5e-4 and the visibility margins are 8e-6 or more at
every radius; seed 3 comes to 1.4e-6 and is not used."""
import ctypes

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import depth_scenes as DS
from tests import fuse_depth_ref as FR
from tests import render_points_ref as RR
from tests import render_scenes as RS
from tests.helpers import kernel_resources

DEV = "cuda:0"
POINTS_PER_BLOCK, PIXELS_PER_BLOCK = 1024, 4096                    # csrc/render_points.hip
EXACT = ("index", "visible", "num_views", "counts")


def _bit(visible, v):
    return (visible.view(np.uint32) >> np.uint32(v)) & 1 == 1


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_covers_its_points_and_hides_what_the_scene_hides(seed):
    """At radius 0 every projection inside a map covers its pixel, a pixel's depth is the fp32 depth of the point it names, and a point
    is never hidden from a view in which it won a pixel.  At radius 1 every projection that the analytic scene puts more than 20 % behind
    the surface on its ray is reported hidden: 89 of 89, 99 of 99 and 109 of 109 at seeds 0, 1, 2.  At radius 0 with depth_tol = 0.05
    only 72, 86 and 94 of those are (81 to 87 %): the holes between the splats of a resampled surface let hidden points through."""
    sc = RS.scene(3, seed)
    ref, V = sc["ref"], 4
    for v in range(V):
        n = np.flatnonzero(ref["inside"][v])
        i, j = ref["row"][v, n], ref["col"][v, n]
        assert (ref["index"][v, i, j] >= 0).all() and (ref["depth"][v, i, j] <= ref["z32"][v, n]).all()
        won = ref["index"][v] >= 0
        winners = ref["index"][v][won]
        assert np.array_equal(ref["depth"][v][won], ref["z32"][v, winners]) and ref["inside"][v, winners].all()
        assert _bit(ref["visible"], v)[winners].all()
        assert not ref["depth"][v][~won].any()
    assert ref["counts"][0] == ref["inside"].sum() and ref["counts"][2] == ref["num_views"].sum() and ref["counts"][3] == 0
    hidden = RS.hidden_projections(sc)
    caught = {}
    for radius in (0, 1):
        vis = RS.scene(3, seed, radius=radius)["ref"]["visible"]
        caught[radius] = sum(int((~_bit(vis, v))[hidden[v]].sum()) for v in range(V))
    print(f"seed {seed}: {int(hidden.sum())} hidden projections, {caught[0]} caught at radius 0, {caught[1]} at radius 1")
    assert int(hidden.sum()) == (89, 99, 109)[seed] and caught[1] == int(hidden.sum())
    assert 0.81 <= round(caught[0] / hidden.sum(), 2) <= 0.87


def _call(lib, a, **kw):
    args = dict(points=a, mask=None, N=8, K=a, R=a, t=a, V=2, H=4, W=6, radius=1, tol=0.05, depth=a, index=a, visible=a, num=a, counts=a,
                ws=a, ws_bytes=1 << 20)
    args.update(kw)
    return lib.roma_render_points(args["points"], args["mask"], args["N"], args["K"], args["R"], args["t"], args["V"], args["H"], args["W"],
                                  args["radius"], args["tol"], args["depth"], args["index"], args["visible"], args["num"], args["counts"],
                                  args["ws"], args["ws_bytes"], None)


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    for kw in ("points", "K", "R", "t", "depth", "index", "visible", "num", "counts", "ws"):
        assert _call(lib, a, **{kw: None}) == _lib.ROMA_E_ARG and b"roma_render_points: null pointer" in lib.roma_last_error(), kw
    for V in (0, 33):
        assert _call(lib, a, V=V) == _lib.ROMA_E_SHAPE and b"roma_render_points: bad shape V=" in lib.roma_last_error()
        assert lib.roma_render_points_workspace(V, 4, 6, None) == _lib.ROMA_E_SHAPE
        assert b"roma_render_points_workspace: bad shape V=" in lib.roma_last_error()
    for H, W in ((0, 6), (4, 0), (32769, 6), (4, 32769)):
        assert _call(lib, a, H=H, W=W) == _lib.ROMA_E_SHAPE and f"bad shape maps of {H}x{W}".encode() in lib.roma_last_error()
        assert lib.roma_render_points_workspace(2, H, W, None) == _lib.ROMA_E_SHAPE
        assert f"roma_render_points_workspace: bad shape maps of {H}x{W}".encode() in lib.roma_last_error()
    assert _call(lib, a, V=2, H=32768, W=32768) == _lib.ROMA_E_SHAPE and b"2^31 - 1 pixels" in lib.roma_last_error()       # 2^31 exactly
    assert lib.roma_render_points_workspace(2, 32768, 32768, None) == _lib.ROMA_E_SHAPE and b"2^31 - 1 pixels" in lib.roma_last_error()
    assert lib.roma_render_points_workspace(1, 32768, 32768, None) == 8 << 30
    for N in (0, -1, 1 << 31):
        assert _call(lib, a, N=N) == _lib.ROMA_E_SHAPE and b"bad shape N=" in lib.roma_last_error()
    for radius in (-1, 5):
        assert _call(lib, a, radius=radius) == _lib.ROMA_E_ARG and b"radius must be in [0, 4]" in lib.roma_last_error()
    for tol in (-1e-9, float("nan"), float("inf")):
        assert _call(lib, a, tol=tol) == _lib.ROMA_E_ARG and b"depth_tol must be finite and not negative" in lib.roma_last_error()
    assert _call(lib, a, points=ctypes.c_void_p(ctypes.addressof(buf) + 2)) == _lib.ROMA_E_ALIGN and b"4-byte" in lib.roma_last_error()
    assert _call(lib, a, ws_bytes=100) == _lib.ROMA_E_ARG and b"workspace of 100 bytes, 512 needed" in lib.roma_last_error()
    assert _call(lib, a, ws=ctypes.c_void_p(ctypes.addressof(buf) + 8)) == _lib.ROMA_E_ALIGN and b"16-byte" in lib.roma_last_error()


def test_workspace_is_the_keys_rounded_up_to_256_bytes():
    """8 bytes per pixel of every map, one region rounded up to 256; the counters are the `counts` output itself"""
    lib = _lib.load()
    size = (ctypes.c_long * 1)()
    need = lib.roma_render_points_workspace(32, 864, 864, ctypes.cast(size, ctypes.c_void_p))
    assert need == -(-8 * 32 * 864 * 864 // 256) * 256 == size[0] == 191_102_976
    assert lib.roma_render_points_workspace(3, 5, 7, None) == 1024      # 840 bytes of keys
    from roma_amd import geometry
    assert geometry.render_points_workspace(3, 5, 7) == 1024
    with pytest.raises(ValueError, match="bad shape"):
        geometry.render_points_workspace(33, 5, 7)


def test_wrapper_validates_before_it_looks_at_a_tensor():
    from roma_amd import geometry
    pts = torch.ones(5, 3)
    R, t, K = torch.eye(3).expand(2, 3, 3), torch.zeros(2, 3), torch.eye(3)
    ok = dict(points=pts, R=R, t=t, K=K, shape=(4, 6))
    for bad in (dict(shape=(4,)), dict(shape=7), dict(shape=(0, 6)), dict(shape=(4, 32769)), dict(radius=-1), dict(radius=5), dict(radius=1.5),
                dict(radius="wide"), dict(depth_tol=-0.1), dict(depth_tol=float("nan")), dict(depth_tol=float("inf")),
                dict(points=torch.ones(5, 2)), dict(points=torch.ones(5)), dict(points=torch.ones(0, 3)), dict(points=[[0.0, 0.0, 1.0]]),
                dict(R=torch.eye(3).expand(33, 3, 3), t=torch.zeros(33, 3)), dict(R=torch.eye(4)), dict(t=torch.zeros(3, 3)),
                dict(t=torch.zeros(3)), dict(R=torch.eye(3), t=torch.zeros(1, 3)), dict(K=torch.eye(3).expand(3, 3, 3)), dict(K=torch.eye(4)),
                dict(sizes=[(4, 6)]), dict(sizes=[(4, 6), (0, 6)]), dict(sizes=7), dict(mask=torch.ones(4, dtype=torch.bool)),
                dict(mask=torch.ones(5)), dict(mask=[1] * 5), dict(attributes=torch.ones(4, 2)), dict(attributes=torch.ones(5)),
                dict(shape=(32768, 32768), R=torch.eye(3).expand(2, 3, 3))):
        args = {**ok, **bad}
        with pytest.raises(ValueError):
            geometry.render_points(args.pop("points"), args.pop("R"), args.pop("t"), args.pop("K"), args.pop("shape"), **args)
    for extra in (dict(), dict(mask=torch.ones(5, dtype=torch.bool)), dict(attributes=torch.ones(5, 2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            geometry.render_points(pts, R, t, K, (4, 6), **extra)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.render_points(pts, torch.eye(3), torch.zeros(3), K, (4, 6))


def test_render_points_kernels_resource_report():
    """The compiler's resource report of csrc/render_points.hip (the table of DESIGN.md §3.4): four kernels, none with scratch"""
    kernels = kernel_resources("render_points.hip")
    names = ("clear", "splat", "resolve", "visible")
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch | occupancy |")
    for n in names:
        (k,) = [v for name, v in kernels.items() if f"render_{n}_kernel" in name]
        print(f"| `render_{n}_kernel` | {k['VGPRs']} | {k['TotalSGPRs']} | {k['LDS Size']} | {k['ScratchSize']} | {k['Occupancy']} |")
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
        assert k["LDS Size"] <= 4096
    assert len(kernels) == len(names), sorted(kernels)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _run(points, R, t, K, shape, mask=None, attributes=None, **kw):
    from roma_amd import geometry
    out = geometry.render_points(_dev(points), _dev(R), _dev(t), _dev(K), shape, mask=None if mask is None else _dev(mask),
                                 attributes=None if attributes is None else _dev(attributes), **kw)
    torch.cuda.synchronize()
    assert type(out).__name__ == "RenderedViews" and out._fields == ("depth", "index", "visible", "num_views", "counts", "attributes")
    return {k: (None if a is None else a.cpu().numpy()) for k, a in out._asdict().items()}


def _ulp_close(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    ulp = np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got))).astype(np.float64)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp


def _compare(got, ref):
    for name in EXACT:
        assert got[name].dtype == ref[name].dtype and got[name].shape == ref[name].shape, name
        assert np.array_equal(got[name], ref[name]), (name, int((got[name] != ref[name]).sum()))
    assert got["depth"].dtype == np.float32 and got["depth"].shape == ref["depth"].shape
    assert _ulp_close(got["depth"], ref["depth"]).all() and not got["depth"][ref["index"] < 0].any()


def _check(points, R, t, K, shape, what, mask=None, **kw):
    """the restatement with its margins asserted, then the device against it"""
    ref = RR.render_points_ref(points, R, t, K, shape, mask=mask, **kw)
    RS.assert_margins(ref, what)
    got = _run(points, R, t, K, shape, mask=mask, **kw)
    _compare(got, ref)
    return got, ref


def _check_scene(sc):
    got = _run(sc["points"], sc["R"], sc["t"], sc["K"], sc["shape"], radius=sc["radius"], depth_tol=sc["depth_tol"])
    _compare(got, sc["ref"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("Vs,seed,radius", [(3, s, r) for s in (0, 1, 2) for r in (0, 1, 2)] + [(5, 0, 1)])
def test_matches_the_restatement(Vs, seed, radius):
    sc = RS.scene(Vs, seed, radius=radius)
    got = _check_scene(sc)
    assert got["counts"][0] > 2000 * Vs and got["counts"][1] > 0.98 * (Vs + 1) * 768 and (got["num_views"] < Vs + 1).any()


@pytest.mark.gpu
def test_one_view_given_as_a_single_pose():
    sc = RS.scene(3, 0)
    K, R, t = sc["K"][3], sc["R"][3], sc["t"][3]
    got, ref = _check(sc["points"], R, t, K, sc["shape"], "single pose", radius=1)
    assert got["depth"].shape == (1, 24, 32) and got["counts"][1] > 700 and set(np.unique(got["visible"])) <= {0, 1}
    assert np.array_equal(got["index"][0], RS.scene(3, 0, radius=1)["ref"]["index"][3])


@pytest.mark.gpu
def test_thirty_two_views_use_bit_31():
    sc = RS.scene(31, 0, shape=(8, 12))
    got = _check_scene(sc)
    assert (got["visible"] < 0).any() and got["num_views"].max() > 16 and (got["index"][31] >= 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 1023, 1024, 1025, 2250])
def test_point_block_edges(N):
    """one below, equal to and one above the points of a block, and a count that spans three blocks"""
    assert N in (1, POINTS_PER_BLOCK - 1, POINTS_PER_BLOCK, POINTS_PER_BLOCK + 1, 2250)
    sc = RS.scene(3, 0)
    got, _ = _check(sc["points"][:N], sc["R"], sc["t"], sc["K"], sc["shape"], f"N={N}", radius=1)
    assert got["visible"].shape == (N,) and got["counts"][0] >= N and 0 <= got["index"].max() < N


@pytest.mark.gpu
@pytest.mark.parametrize("Vs,shape", [(2, (1, 1)), (2, (31, 33)), (2, (32, 32)), (2, (45, 50)), (2, (35, 39)), (1, (32, 64)), (1, (33, 63))])
def test_pixel_block_edges(Vs, shape):
    """maps of 1, 1 023, 1 024 and 2 250 pixels; and, since one block resolves 4 096 pixels of all maps together, 4 095, 4 096 and 4 158"""
    words = (Vs + 1) * shape[0] * shape[1]
    assert words in (3, 3 * 1023, 3 * 1024, 3 * 2250, PIXELS_PER_BLOCK - 1, PIXELS_PER_BLOCK, PIXELS_PER_BLOCK + 62)
    sc = RS.scene(Vs, 0, shape=shape, radius=1)
    got = _check_scene(sc)
    assert got["counts"][1] > 0.9 * words


IDENTITY_K = np.array([[10.0, 0.0, 5.0], [0.0, 10.0, 5.0], [0.0, 0.0, 1.0]])


@pytest.mark.gpu
def test_equal_depths_in_one_pixel_go_to_the_lowest_index():
    """Under R = I, t = 0 and a K without skew and with k22 = 1, q.z is X.z exactly on the device and in the restatement.  Rows 3, 5, 6
    and 9 lie at z = 2 at different places of pixel (5, 5); rows 0 and 7 are farther in the same pixel, row 1 is nearer in another."""
    z = np.array([2.5, 1.5, 3.0, 2.0, 4.0, 2.0, 2.0, 2.25, 3.5, 2.0])
    u = np.array([5.3, 7.4, 1.2, 5.81, 8.3, 5.12, 5.47, 5.66, 2.2, 5.33])
    w = np.array([5.6, 2.3, 8.1, 5.17, 0.4, 5.72, 5.38, 5.21, 3.3, 5.9])
    pts = np.stack([(u - 5.0) / 10.0 * z, (w - 5.0) / 10.0 * z, z], -1).astype(np.float32)
    for radius in (0, 1):
        got, ref = _check(pts, np.eye(3), np.zeros(3), IDENTITY_K, (10, 10), "ties", radius=radius)
        assert got["index"][0, 5, 5] == 3 and got["depth"][0, 5, 5] == 2.0 and np.array_equal(got["depth"], ref["depth"])
        assert got["visible"][[3, 5, 6, 9]].all() and not got["visible"][[0, 7]].any()
    assert got["index"][0, 4, 4] == 3 and got["index"][0, 2, 7] == 1 and got["index"][0, 3, 6] == 1


@pytest.mark.gpu
def test_exact_duplicates_go_to_the_lowest_index():
    sc = RS.scene(3, 0)
    pts = np.concatenate([sc["points"][700:1000], sc["points"]])           # rows 0 .. 299 are rows 1000 .. 1299 again
    got, ref = _check(pts, sc["R"], sc["t"], sc["K"], sc["shape"], "duplicates", radius=1)
    assert ((got["index"] >= 1000) & (got["index"] < 1300)).sum() == 0 and ((got["index"] >= 0) & (got["index"] < 300)).sum() > 300
    assert np.array_equal(got["visible"][:300], got["visible"][1000:1300])


@pytest.mark.gpu
def test_4096_points_on_one_ray_contend_for_one_pixel():
    sc = RS.scene(3, 0)
    K, R, t = sc["K"][1], sc["R"][1], sc["t"][1]
    rng = np.random.default_rng(11)
    lam = 3.0 + 1.0007e-3 * rng.permutation(4096)
    ray = np.linalg.inv(K) @ np.array([10.5, 7.5, 1.0])
    pts = ((lam[:, None] * ray - t) @ R).astype(np.float32)
    got, ref = _check(pts, R, t, K, sc["shape"], "one ray")
    assert ref["inside"].all() and (ref["row"] == 7).all() and (ref["col"] == 10).all()
    assert got["counts"][0] == 4096 and got["counts"][1] == 1 and got["counts"][2] == 150             # 5 % of 3.0 is 149.9 steps
    assert got["index"][0, 7, 10] == int(np.argmin(lam)) and (got["index"] >= 0).sum() == 1
    assert got["depth"][0, 7, 10] == ref["z32"][0].min()


def _pixel_points(pix, z, K):
    pix, z = np.asarray(pix, np.float64), np.asarray(z, np.float64)
    rays = np.concatenate([pix, np.ones((len(pix), 1))], -1) @ np.linalg.inv(K).T
    return (rays * z[:, None]).astype(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,radius", [((9, 11), 1), ((9, 11), 2), ((9, 11), 4), ((3, 3), 4), ((1, 7), 3)])
def test_footprints_are_clipped_at_edges_and_corners(shape, radius):
    """a point in every pixel within `radius` of an edge — the corners included — each at a depth of its own"""
    H, W = shape
    K = np.array([[8.0, 0.1, W / 2 + 0.3], [0.0, 7.0, H / 2 - 0.2], [0.0, 0.0, 1.0]])
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    rim = (np.minimum(ii, H - 1 - ii) < radius) | (np.minimum(jj, W - 1 - jj) < radius)
    pix = np.stack([jj[rim] + 0.37, ii[rim] + 0.61], -1)
    rng = np.random.default_rng(5)
    pts = _pixel_points(pix, 2.0 + 0.0137 * rng.permutation(len(pix)), K)
    got, ref = _check(pts, np.eye(3), np.zeros(3), K, shape, f"clipping {shape} {radius}", radius=radius)
    assert got["counts"][0] == len(pts) and (got["index"][0][rim] >= 0).all()
    reach = np.minimum(np.minimum(ii, H - 1 - ii), np.minimum(jj, W - 1 - jj)) < 2 * radius      # a rim pixel within `radius`
    assert np.array_equal(got["index"][0] >= 0, reach)
    if shape == (3, 3):
        assert (got["index"] == int(np.argmin(pts[:, 2]))).all()         # every footprint covers the whole map


@pytest.mark.gpu
def test_rows_that_are_not_drawn():
    """NaN, +inf and -inf coordinates, masked rows, rows behind the camera, coordinates of 1e30, and 3e38 on the axis of a view whose K is
    scaled by 2 (the same camera), where q.z = 6e38 is finite in fp64 and overflows fp32: none is drawn, none is seen, the rest is as
    it would be without them; only the masked and the non-finite rows count as not live."""
    sc = RS.scene(3, 0)
    pts = sc["points"].copy()
    K = sc["K"].copy()
    K[0] *= 2.0
    N = len(pts)
    mask = np.ones(N, np.uint8)
    bad = {"nan": [3, 800], "inf": [40, 1500], "ninf": [77], "masked": [5, 6, 900, 2303], "behind": [100, 1700], "far": [200, 201], "axis": [300]}
    pts[3, 0] = pts[800, 2] = np.nan
    pts[40, 1] = pts[1500] = np.inf
    pts[77, 2] = -np.inf
    mask[bad["masked"]] = 0
    pts[100] = [0.1, -0.2, -6.0]
    pts[1700] = [0.0, 0.0, -2.0]
    pts[200] = [1e30, 1e30, 1e30]
    pts[201] = [-1e30, 2e30, 1e30]
    pts[300] = [0.0, 0.0, 3e38]
    got, ref = _check(pts, sc["R"], sc["t"], K, sc["shape"], "bad rows", mask=mask, radius=1)
    gone = sum((rows for kind, rows in bad.items() if kind != "axis"), [])             # the other views draw row 300 where it is finite
    assert not np.isin(got["index"], gone).any() and not (got["index"][0] == 300).any() and np.isfinite(got["depth"]).all()
    assert got["counts"][3] == 9 and not ref["live"][bad["nan"] + bad["inf"] + bad["ninf"] + bad["masked"]].any()
    assert not got["visible"][bad["nan"] + bad["inf"] + bad["ninf"] + bad["masked"] + bad["behind"]].any()
    q = K[0] @ (sc["R"][0] @ pts[300].astype(np.float64) + sc["t"][0])
    with np.errstate(over="ignore"):
        assert np.isfinite(q).all() and 0 <= q[0] / q[2] < 32 and 0 <= q[1] / q[2] < 24 and np.isinf(q[2].astype(np.float32))
    assert not _bit(got["visible"], 0)[300] and not ref["inside"][0, 300]
    # as a bool mask, and all rows masked
    got_b = _run(pts, sc["R"], sc["t"], K, sc["shape"], mask=mask.astype(bool), radius=1)
    assert all(np.array_equal(got_b[k], got[k]) for k in EXACT + ("depth",))
    none = _run(pts, sc["R"], sc["t"], K, sc["shape"], mask=np.zeros(N, bool), radius=1)
    assert none["counts"].tolist() == [0, 0, 0, N] and (none["index"] == -1).all() and not none["depth"].any() and not none["visible"].any()
    assert not none["num_views"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["singular_k", "lower_k", "nan_t"])
def test_an_unusable_view_in_the_middle(how):
    sc = RS.scene(3, 0, radius=1)
    K, t = sc["K"].copy(), sc["t"].copy()
    if how == "singular_k":
        K[1, 0, 0] = 0.0
    elif how == "lower_k":
        K[1, 1, 0] = 1e-3
    else:
        t[1, 2] = np.nan
    got, ref = _check(sc["points"], sc["R"], t, K, sc["shape"], how, radius=1)
    assert not ref["usable"][1] and (got["index"][1] == -1).all() and not got["depth"][1].any() and not _bit(got["visible"], 1).any()
    for v in (0, 2, 3):
        assert np.array_equal(got["index"][v], sc["ref"]["index"][v]) and np.array_equal(_bit(got["visible"], v), _bit(sc["ref"]["visible"], v))


@pytest.mark.gpu
def test_sizes_scale_the_intrinsics_per_axis():
    """maps of 24 x 32 with the K of images of 48 x 64 and of 72 x 64: the same as K scaled by hand, bit for bit"""
    V, shape = 3, (24, 32)
    sizes = [(48, 64), (72, 64), (48, 96)]
    K, R, t = DS.cameras(V, 0, (48, 64))
    K[1, 1] *= 1.5
    K[2, 0] *= 1.5
    Kmap = RR.scaled_intrinsics(K, V, shape, sizes)
    pts = RS.cloud_of(Kmap, R, t, shape, range(2))
    got, _ = _check(pts, R, t, K, shape, "sizes", sizes=sizes, radius=1)
    by_hand = _run(pts, R, t, Kmap, shape, radius=1)
    assert all(np.array_equal(got[k], by_hand[k]) for k in EXACT + ("depth",)) and got["counts"][1] > 2000


@pytest.mark.gpu
def test_attributes_are_gathered_through_the_index():
    sc = RS.scene(3, 0)
    rng = np.random.default_rng(2)
    colour = rng.integers(1, 255, size=(len(sc["points"]), 3)).astype(np.uint8)
    feat = rng.normal(size=(len(sc["points"]), 5)).astype(np.float32)
    for attr in (colour, feat):
        got = _run(sc["points"], sc["R"], sc["t"], sc["K"], sc["shape"], attributes=attr)
        _compare(got, sc["ref"])
        holes = sc["ref"]["index"] < 0
        assert holes.sum() > 20 and got["attributes"].shape == (4, 24, 32, attr.shape[1]) and got["attributes"].dtype == attr.dtype
        assert np.array_equal(got["attributes"][~holes], attr[sc["ref"]["index"][~holes]]) and not got["attributes"][holes].any()


@pytest.mark.gpu
def test_order_of_arrival_changes_nothing():
    """no two candidates of a pixel of this scene have the same fp32 depth (asserted), so every winner is decided by depth alone: the
    cloud permuted at random gives bit-identical depth, index mapped through the permutation and visible permuted; two calls and a
    graph replay are bit-identical"""
    from roma_amd import geometry
    sc = RS.scene(3, 0, radius=1)
    ref = sc["ref"]
    RS.assert_no_ties(ref, sc["shape"], 1)
    got = _check_scene(sc)
    perm = np.random.default_rng(9).permutation(len(sc["points"]))
    mixed = _run(sc["points"][perm], sc["R"], sc["t"], sc["K"], sc["shape"], radius=1)
    assert np.array_equal(mixed["depth"].view(np.uint32), got["depth"].view(np.uint32))
    assert np.array_equal(np.where(mixed["index"] >= 0, perm[np.maximum(mixed["index"], 0)], -1), got["index"])
    assert np.array_equal(mixed["visible"], got["visible"][perm]) and np.array_equal(mixed["counts"], got["counts"])

    pts, R, t, K = _dev(sc["points"]), _dev(sc["R"]), _dev(sc["t"]), _dev(sc["K"])
    attr = _dev(np.arange(len(sc["points"]), dtype=np.float32)[:, None])

    def call():
        return tuple(geometry.render_points(pts, R, t, K, sc["shape"], radius=1, attributes=attr))

    def same(a, b):
        return all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))

    first, second = call(), call()
    assert same(first, second) and np.array_equal(first[1].cpu().numpy(), ref["index"])
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
def test_chain_fused_cloud_drawn_into_a_held_out_view():
    """fuse_depth_maps on three perturbed 24 x 32 maps with the K of the 48 x 64 images, the cloud (tail rows masked by pixel >= 0) drawn
    at radius 1 into a fourth view that contributed nothing, and lift_keypoints at the centres of the covered pixels.  The restatement,
    run on the device's cloud, gives the three figures and the device must reproduce them.  Measured on an MI355X: see DESIGN.md §3.4."""
    from roma_amd import geometry
    shape, image = (24, 32), (48, 64)
    sc = DS.fuse_scene(3, 0, images=(image,))
    K4, R4, t4 = DS.cameras(4, 0, image)
    assert np.array_equal(K4[:3], sc["K"]) and np.array_equal(R4[:3], sc["R"])
    T = int(sc["ref"]["counts"][0]) + 7
    fused = geometry.fuse_depth_maps([_dev(d) for d in sc["depths"]], _dev(sc["R"]), _dev(sc["t"]), _dev(sc["K"]), sizes=sc["sizes"],
                                     max_points=T)
    live = fused.pixel >= 0
    out = geometry.render_points(fused.points, _dev(R4[3]), _dev(t4[3]), _dev(K4[3]), shape, sizes=[image], mask=live, radius=1)
    torch.cuda.synchronize()
    n_fused = int(fused.counts[0])
    assert n_fused == T - 7 and int(live.sum()) == n_fused
    cloud, mask = fused.points.cpu().numpy(), live.cpu().numpy()
    ref = RR.render_points_ref(cloud, R4[3], t4[3], K4[3], shape, sizes=[image], radius=1, mask=mask)
    RS.assert_margins(ref, "chain")
    _compare({k: getattr(out, k).cpu().numpy() for k in EXACT + ("depth",)}, ref)
    assert out.index.max() < n_fused and int(out.counts[3]) == 7                       # no tail row is drawn
    Kmap = RR.scaled_intrinsics(K4[3], 1, shape, [image])[0]
    truth, _ = DS.render(Kmap, R4[3], t4[3], shape)

    def figures(depth):
        ii, jj = np.nonzero(depth > 0)
        d = depth[ii, jj].astype(np.float64)
        X = FR.lift(jj + 0.5, ii + 0.5, d, np.linalg.inv(Kmap), R4[3], t4[3])
        return len(ii) / depth.size, np.median(np.abs(d - truth[ii, jj]) / truth[ii, jj]), np.median(DS.surface_distance(X))

    want = figures(ref["depth"][0])
    depth = out.depth[0]
    ii, jj = torch.nonzero(depth > 0, as_tuple=True)
    kp = torch.stack([jj + 0.5, ii + 0.5], -1)
    Xc = geometry.lift_keypoints(kp, depth, _dev(Kmap)).cpu().numpy()                  # in the frame of the held-out camera
    Xw = (Xc - t4[3]) @ R4[3]
    d = depth[ii, jj].double().cpu().numpy()
    got = (len(d) / depth.numel(), np.median(np.abs(d - truth[ii.cpu().numpy(), jj.cpu().numpy()]) / truth[ii.cpu().numpy(), jj.cpu().numpy()]),
           np.median(DS.surface_distance(Xw)))
    print(f"chain: {n_fused} fused points; coverage {want[0]:.4f}, median relative depth error {want[1]:.2e}, median distance of the lifted "
          f"points to the surface {want[2]:.2e} (restatement); device {got[0]:.4f}, {got[1]:.2e}, {got[2]:.2e}")
    # a device depth is within one fp32 ulp of the restatement's: 2^-23 relative, and 2^-23 of a depth below 16 along the ray
    assert got[0] == want[0] and np.isfinite(Xw).all()
    assert abs(got[1] - want[1]) <= 2.0 ** -23 and abs(got[2] - want[2]) <= 16 * 2.0 ** -23
