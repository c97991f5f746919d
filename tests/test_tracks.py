"""build_tracks (csrc/tracks.hip): multi-view tracks from pairwise matches.

tests/tracks_ref.py restates the definition in numpy.  The kernels use integer atomics that commute and nothing else that depends on
the order of arrival, so every output is compared with the restatement for EQUALITY (x with its NaN pattern); the one tolerance in
this file is the 5 % of the last test, which compares two triangulations.  Every GPU test asserts the status word 0.

The scenes are tests/multiview_scenes.multiview_scene(V, seed, N=400, outlier_frac=0.0): all pairs a < b with k = 400, the endpoints
of match j the scene's observations of point j normalised in fp32 as x / (W/2) - 1, certainty uniform in (0.1, 1) where both views
see the point and 0 elsewhere, cell = 4."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from roma_amd import _lib
from tests import multiview_scenes as MS
from tests import tracks_ref as TR
from tests.helpers import kernel_resources

DEV = "cuda:0"
FIELDS = ("x", "visible", "views", "num_views", "track_of_match", "counts")
T_FULL = 512                                                       # above the number of tracks of every scene here


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def scene(V, seed):
    return MS.multiview_scene(V, seed, N=400, outlier_frac=0.0)


@functools.lru_cache(maxsize=None)
def scene_inputs(V, seed):
    """the matches of the module docstring: matches (M,400,4), certainty (M,400), pairs (M,2), sizes as (H, W)"""
    s = scene(V, seed)
    sizes = tuple((int(h), int(w)) for w, h in s["sizes"])
    half = np.array([[w / 2, h / 2] for h, w in sizes], np.float32)
    norm = s["x"] / half[:, None, :] - np.float32(1)
    assert norm.dtype == np.float32
    pairs = np.array([(a, b) for a in range(V) for b in range(a + 1, V)], np.int32)
    matches = np.stack([np.concatenate([norm[a], norm[b]], -1) for a, b in pairs])
    both = np.stack([s["seen"][a] & s["seen"][b] for a, b in pairs])
    rng = np.random.default_rng([seed, 23])
    certainty = np.where(both, rng.uniform(0.1, 1.0, both.shape), 0.0).astype(np.float32)
    return _frozen(matches=matches, certainty=certainty, pairs=pairs, sizes=sizes)


@functools.lru_cache(maxsize=None)
def scene_ref(V, seed, max_tracks=T_FULL):
    return _frozen(**TR.build_tracks_ref(**scene_inputs(V, seed), cell=4, max_tracks=max_tracks))


def pure_tracks(out, s, k=400):
    """[(row, point)] of the tracks whose visible set is the point's `seen` column and whose pixels are its observations to 1e-2 px"""
    tom = out["track_of_match"].reshape(-1)
    rows, first = np.unique(tom, return_index=True)
    found = []
    for r, i in zip(rows, first):
        if r < 0:
            continue
        j = int(i) % k
        vis = out["visible"][:, r]
        if (vis == s["seen"][:, j]).all() and np.abs(out["x"][vis, r] - s["x"][vis, j]).max() <= 1e-2:
            found.append((int(r), j))
    assert len({j for _, j in found}) == len(found)
    return found


def norm_px(px, size):
    """pixels -> normalised coordinates in fp32, as the scenes do"""
    return (np.asarray(px, np.float32) / np.float32(size / 2) - np.float32(1)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_recovers_the_scene_points_as_pure_tracks(seed):
    s, out = scene(5, seed), scene_ref(5, seed)
    seen2 = int((s["seen"].sum(0) >= 2).sum())
    pure = pure_tracks(out, s)
    print(f"seed {seed}: {len(pure)} pure tracks of {seen2} points seen in two or more views ({100 * len(pure) / seen2:.1f} %), counts {out['counts']}")
    assert out["counts"][0] < T_FULL and len(pure) >= 0.9 * seen2


def test_restatement_does_not_depend_on_the_order_of_pairs_and_matches():
    inp, want = scene_inputs(5, 0), scene_ref(5, 0)
    live = inp["certainty"][inp["certainty"] > 0]
    assert len(np.unique(live)) == len(live)                         # all distinct: no tie to break by position
    rng = np.random.default_rng(5)
    order = rng.permutation(len(inp["pairs"]))
    within = np.stack([rng.permutation(400) for _ in order])
    m = np.take_along_axis(inp["matches"][order], within[..., None], 1)
    c = np.take_along_axis(inp["certainty"][order], within, 1)
    got = TR.build_tracks_ref(m, c, inp["pairs"][order], inp["sizes"], cell=4, max_tracks=T_FULL)
    for name in ("x", "visible", "views", "num_views", "counts"):
        assert np.array_equal(got[name], want[name], equal_nan=name == "x"), name
    back = np.empty_like(got["track_of_match"])
    np.put_along_axis(back, within, got["track_of_match"], 1)
    assert np.array_equal(back[np.argsort(order)], want["track_of_match"])


def _tiny(rows, k, pairs, sizes=((16, 16),) * 3):
    """rows: (pair, slot, (xA, yA), (xB, yB), certainty) in pixels -> matches, certainty; untouched slots have certainty 0"""
    m = np.zeros((len(pairs), k, 4), np.float32)
    c = np.zeros((len(pairs), k), np.float32)
    for p, j, A, B, cert in rows:
        a, b = pairs[p]
        m[p, j] = [norm_px(A[0], sizes[a][1]), norm_px(A[1], sizes[a][0]), norm_px(B[0], sizes[b][1]), norm_px(B[1], sizes[b][0])]
        c[p, j] = cert
    return m, c


def test_restatement_breaks_a_certainty_tie_by_the_lowest_endpoint_index():
    pairs = [(0, 1)]
    m, c = _tiny([(0, 0, (1.25, 1.5), (9.5, 9.5), 0.5), (0, 1, (2.75, 2.5), (9.25, 9.75), 0.5), (0, 2, (3.5, 3.5), (9.0, 9.0), 0.25)], 3, pairs)
    out = TR.build_tracks_ref(m, c, pairs, [(16, 16)] * 2, cell=4, max_tracks=4)
    assert tuple(out["counts"]) == (1, 0, 0, 0) and (out["track_of_match"] == 0).all()
    assert np.array_equal(out["x"][:, 0], np.array([[1.25, 1.5], [9.5, 9.5]], np.float32))
    out = TR.build_tracks_ref(m[:, ::-1], c[:, ::-1], pairs, [(16, 16)] * 2, cell=4, max_tracks=4)
    assert np.array_equal(out["x"][:, 0], np.array([[2.75, 2.5], [9.25, 9.75]], np.float32))


def test_restatement_two_points_sharing_a_cell_conflict():
    pairs = [(0, 1)]
    m, c = _tiny([(0, 0, (1.5, 1.5), (1.5, 1.5), 0.9), (0, 1, (2.5, 2.5), (9.5, 9.5), 0.8)], 2, pairs)
    out = TR.build_tracks_ref(m, c, pairs, [(16, 16)] * 2, cell=4, max_tracks=4)
    assert tuple(out["counts"]) == (0, 1, 0, 0) and (out["track_of_match"] == -1).all()
    assert np.isnan(out["x"]).all() and not out["visible"].any() and not out["views"].any()


def _four_ways_to_minus_one():
    """three views, cell 4, min_views 3, max_tracks 2: tracks at cells (0,0), (2,2), (3,3) over all three views — the third is beyond
    max_tracks —, a two-view component at cell (1,1), a conflict around cell (0,3) of view 0, and slots that are not usable"""
    pairs = [(0, 1), (1, 2), (0, 2)]
    rows = []
    for slot, at in enumerate((1.5, 9.5, 13.5)):
        rows += [(0, slot, (at, at), (at, at), 0.9), (1, slot, (at, at), (at, at), 0.8)]
    rows += [(0, 3, (5.5, 5.5), (5.5, 5.5), 0.7)]                                         # two views only
    rows += [(2, 0, (1.5, 13.5), (1.5, 13.5), 0.6), (2, 1, (2.5, 14.5), (9.5, 13.5), 0.6), (1, 3, (1.5, 13.5), (1.5, 13.5), 0.6)]   # conflict
    m, c = _tiny(rows, 6, pairs)
    m[0, 4], c[0, 4] = [0.0, 0.0, 1.0, 0.0], 0.9                                          # x_B = 1.0: outside
    m[2, 2], c[2, 2] = [0.0, 0.0, np.nan, 0.0], 0.9
    want = np.full((3, 6), -1, np.int32)
    want[0, 0] = want[1, 0] = 0
    want[0, 1] = want[1, 1] = 1
    return m, c, np.array(pairs, np.int32), ((16, 16),) * 3, want


def test_restatement_track_of_match_is_minus_one_for_exactly_the_four_reasons():
    m, c, pairs, sizes, want = _four_ways_to_minus_one()
    out = TR.build_tracks_ref(m, c, pairs, sizes, cell=4, min_views=3, max_tracks=2)
    assert tuple(out["counts"]) == (3, 1, 1, 0)
    assert np.array_equal(out["track_of_match"], want)
    assert out["views"].tolist() == [7, 7] and out["num_views"].tolist() == [3, 3] and out["visible"].all()


def _abi_call(lib, a, **kw):
    sizes = (ctypes.c_int * 64)(*([48, 64] * 32))
    arg = dict(matches=a, certainty=a, mask=None, pairs=a, sizes=ctypes.cast(sizes, ctypes.c_void_p), M=4, k=100, V=3, cell=4, thresh=0.0,
               min_views=2, T=16, x=a, visible=a, views=a, num_views=a, tom=a, counts=a, ws=a, ws_size=1 << 40)
    arg.update(kw)
    return lib.roma_build_tracks(arg["matches"], arg["certainty"], arg["mask"], arg["pairs"], arg["sizes"], arg["M"], arg["k"], arg["V"],
                                 arg["cell"], arg["thresh"], arg["min_views"], arg["T"], arg["x"], arg["visible"], arg["views"],
                                 arg["num_views"], arg["tom"], arg["counts"], arg["ws"], arg["ws_size"], None)


def test_entry_points_validate_arguments_without_a_gpu():
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    call = functools.partial(_abi_call, lib, a)
    for name in ("matches", "certainty", "pairs", "sizes", "x", "visible", "views", "num_views", "tom", "counts", "ws"):
        assert call(**{name: None}) == _lib.ROMA_E_ARG and b"roma_build_tracks: null pointer" in lib.roma_last_error(), name
    for kw in ({"V": 1}, {"V": 33}, {"V": 0}):
        assert call(**kw) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error(), kw
    for kw in ({"cell": 0}, {"cell": 65}, {"cell": -4}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"cell must be in [1, 64]" in lib.roma_last_error(), kw
    for kw in ({"min_views": 1}, {"min_views": 4}):
        assert call(**kw) == _lib.ROMA_E_ARG and b"min_views" in lib.roma_last_error(), kw
    for kw in ({"T": 0}, {"T": -1}):
        assert call(**kw) == _lib.ROMA_E_SHAPE and b"max_tracks" in lib.roma_last_error(), kw
    for kw in ({"M": 1 << 16, "k": 1 << 15}, {"M": 0}, {"k": 0}):
        assert call(**kw) == _lib.ROMA_E_SHAPE and b"M * k" in lib.roma_last_error(), kw
    for thresh in (-0.5, float("nan"), float("inf")):
        assert call(thresh=thresh) == _lib.ROMA_E_ARG and b"certainty_thresh" in lib.roma_last_error(), thresh
    huge = (ctypes.c_int * 64)(*([65536, 65536] * 32))
    assert call(sizes=ctypes.cast(huge, ctypes.c_void_p), cell=1) == _lib.ROMA_E_SHAPE and b"use a larger cell" in lib.roma_last_error()
    bad = (ctypes.c_int * 64)(*([48, 0] * 32))
    assert call(sizes=ctypes.cast(bad, ctypes.c_void_p)) == _lib.ROMA_E_SHAPE and b"bad shape of view 0" in lib.roma_last_error()

    sizes = (ctypes.c_int * 6)(48, 64, 17, 23, 33, 19)
    cells = ctypes.c_long(0)
    need = lib.roma_tracks_workspace(3, ctypes.cast(sizes, ctypes.c_void_p), 4, ctypes.byref(cells))
    C = 12 * 16 + 5 * 6 + 9 * 5
    assert cells.value == C == int(TR.grid([(48, 64), (17, 23), (33, 19)], 4)[0][-1])
    assert need >= 21 * C + 12 * -(-C // 256) and need % 16 == 0
    assert call(sizes=ctypes.cast(sizes, ctypes.c_void_p), ws_size=need - 1) == _lib.ROMA_E_SHAPE and b"workspace of" in lib.roma_last_error()
    odd = ctypes.c_void_p(a.value + 4)
    assert call(sizes=ctypes.cast(sizes, ctypes.c_void_p), matches=odd) == _lib.ROMA_E_ALIGN and b"16-byte aligned" in lib.roma_last_error()
    ws = lib.roma_tracks_workspace
    assert ws(3, None, 4, None) == _lib.ROMA_E_ARG and b"roma_tracks_workspace: null pointer" in lib.roma_last_error()
    assert ws(1, ctypes.cast(sizes, ctypes.c_void_p), 4, None) == _lib.ROMA_E_SHAPE and b"bad shape V=" in lib.roma_last_error()
    assert ws(3, ctypes.cast(sizes, ctypes.c_void_p), 0, None) == _lib.ROMA_E_ARG and b"cell must be" in lib.roma_last_error()
    assert ws(32, ctypes.cast(huge, ctypes.c_void_p), 1, None) == _lib.ROMA_E_SHAPE and b"use a larger cell" in lib.roma_last_error()


def test_wrapper_refuses_cpu_tensors_and_bad_arguments():
    from roma_amd import geometry
    m, c, pairs = torch.rand(3, 50, 4) * 2 - 1, torch.rand(3, 50), torch.tensor([[0, 1], [1, 2], [0, 2]], dtype=torch.int32)
    sizes = [(48, 64)] * 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        geometry.build_tracks(m, c, pairs, sizes, max_tracks=16)
    # bad arguments are refused before anything looks at a tensor, mismatched shapes before anything is launched
    for kw, what in (({"cell": 0}, "cell"), ({"cell": 65}, "cell"), ({"min_views": 1}, "min_views"), ({"min_views": 4}, "min_views"),
                     ({"max_tracks": 0}, "max_tracks"), ({"certainty_thresh": -1.0}, "certainty_thresh"),
                     ({"certainty_thresh": float("nan")}, "certainty_thresh")):
        with pytest.raises(ValueError, match=what):
            geometry.build_tracks(m, c, pairs, sizes, **{"max_tracks": 16, **kw})
    for bad_sizes in ([(48, 64)], [(48, 64)] * 33, [(48, 0)] * 3, [48, 64, 3]):
        with pytest.raises(ValueError, match="views|sizes"):
            geometry.build_tracks(m, c, pairs, bad_sizes, max_tracks=16)
    with pytest.raises(ValueError, match="larger cell"):
        geometry.build_tracks(m, c, pairs, [(65536, 65536)] * 3, cell=4, max_tracks=16)          # a workspace above 2 GiB
    with pytest.raises(ValueError, match="larger cell"):
        geometry.build_tracks(m, c, pairs, [(65536, 65536)] * 32, cell=1, max_tracks=16)         # 2^31 cells or more
    for args, what in (((m[..., :3], c, pairs), "matches"), ((m, c[:, :49], pairs), "certainty"), ((m, c, pairs[:2]), "pairs"),
                       ((m, c, pairs.float()), "pairs"), ((m.long(), c, pairs), "matches")):
        with pytest.raises(ValueError, match=what):
            geometry.build_tracks(*args, sizes, max_tracks=16)
    with pytest.raises(ValueError, match="mask"):
        geometry.build_tracks(m, c, pairs, sizes, mask=torch.ones(3, 49, dtype=torch.bool), max_tracks=16)
    assert "Tracks(x=(3, 16, 2)" in repr(geometry.Tracks(torch.zeros(3, 16, 2), None, None, None, torch.zeros(3, 50), None))


def test_tracks_kernels_resource_report():
    """The compiler's resource report of csrc/tracks.hip (the table of DESIGN.md §3.4): eight kernels, none with scratch."""
    kernels = kernel_resources("tracks.hip")
    names = ("init", "endpoints", "union", "flatten", "count", "scan", "rank", "scatter")
    print("| kernel | VGPRs | SGPRs | LDS bytes | scratch | occupancy |")
    for n in names:
        (k,) = [v for name, v in kernels.items() if f"tracks_{n}_kernel" in name]
        print(f"| `tracks_{n}_kernel` | {k['VGPRs']} | {k['TotalSGPRs']} | {k['LDS Size']} | {k['ScratchSize']} | {k['Occupancy']} |")
        assert k["ScratchSize"] == 0 and k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, (n, k)
    assert len(kernels) == len(names), sorted(kernels)


# ------------------------------------------------------------------------------------------------------------------ GPU
def _dev(a):
    return torch.tensor(np.asarray(a), device=DEV)


def _fields(tr):
    out = {name: getattr(tr, name).cpu().numpy() for name in FIELDS}
    assert out["counts"][3] == 0, "the union's retry cap was reached"
    return out


def _run(matches, certainty, pairs, sizes, mask=None, **kw):
    from roma_amd import geometry
    kw.setdefault("max_tracks", T_FULL)
    return _fields(geometry.build_tracks(_dev(matches), _dev(certainty), _dev(pairs), sizes, mask=None if mask is None else _dev(mask), **kw))


def _assert_equal(got, want):
    for name in FIELDS:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name], equal_nan=name == "x"), name


@pytest.mark.gpu
@pytest.mark.parametrize("V,seed", [(5, 0), (5, 1), (5, 2), (8, 0)])
def test_scenes_equal_the_restatement(V, seed):
    want = scene_ref(V, seed)
    got = _run(**scene_inputs(V, seed), cell=4)
    _assert_equal(got, want)
    assert 100 < got["counts"][0] < T_FULL


EDGE_SIZES = ((24, 32), (17, 23), (33, 19))


@functools.lru_cache(maxsize=None)
def edge_inputs(k, cell):
    """one pair, k matches over small views whose sides are no multiples of the cell: match j joins cell (cx, cy) of one view to cell
    (cx, cy) of the other at random places inside them — in a partial last cell some fall outside the image —, 2 % have a stray B end
    anywhere up to 5 % outside, and the certainties come in steps of 1/16 (ties) with zeros"""
    a, b = {1023: (0, 1), 1024: (1, 2), 1025: (2, 0)}[k]
    rng = np.random.default_rng([k, cell])
    (Ha, Wa), (Hb, Wb) = EDGE_SIZES[a], EDGE_SIZES[b]
    cx, cy = rng.integers(0, -(-min(Wa, Wb) // cell), k), rng.integers(0, -(-min(Ha, Hb) // cell), k)
    place = lambda c, size: norm_px((c + rng.uniform(0.01, 0.99, k)) * cell, size)  # noqa: E731
    A = np.stack([place(cx, Wa), place(cy, Ha)], -1)
    B = np.stack([place(cx, Wb), place(cy, Hb)], -1)
    B = np.where(rng.random((k, 1)) < 0.02, rng.uniform(-1.05, 1.05, (k, 2)).astype(np.float32), B)
    matches = np.concatenate([A, B], -1)[None]
    certainty = (rng.integers(0, 17, (1, k)) / 16).astype(np.float32)
    return _frozen(matches=matches, certainty=certainty, pairs=np.array([(a, b)], np.int32), sizes=EDGE_SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("cell", [1, 4, 5])
@pytest.mark.parametrize("k", [1023, 1024, 1025])
def test_workgroup_edges_and_partial_cells(k, cell):
    inp = edge_inputs(k, cell)
    want = TR.build_tracks_ref(**inp, cell=cell, max_tracks=T_FULL)
    got = _run(**inp, cell=cell)
    print(f"k {k} cell {cell}: counts {got['counts']}")
    _assert_equal(got, want)
    assert got["counts"][0] > 0 and got["counts"][1] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_deep_chain_is_one_conflicting_component(order):
    """match j joins cell ceil(j/2) of view 0 to cell floor(j/2) of view 1: one component of 4097 nodes"""
    k = 4096
    j = {"ascending": np.arange(k), "descending": np.arange(k)[::-1], "random": np.random.default_rng(3).permutation(k)}[order]
    ca, cb = (j + 1) // 2, j // 2
    centre = lambda c: np.stack([norm_px(c % 48 + 0.5, 48), norm_px(c // 48 + 0.5, 48)], -1)
    matches = np.concatenate([centre(ca), centre(cb)], -1)[None]
    certainty = np.random.default_rng(4).uniform(0.1, 1.0, (1, k)).astype(np.float32)
    pairs, sizes = np.array([[0, 1]], np.int32), ((48, 48),) * 2
    got = _run(matches, certainty, pairs, sizes, cell=1)
    _assert_equal(got, TR.build_tracks_ref(matches, certainty, pairs, sizes, cell=1, max_tracks=T_FULL))
    assert tuple(got["counts"]) == (0, 1, 0, 0) and (got["track_of_match"] == -1).all() and np.isnan(got["x"]).all()


@pytest.mark.gpu
def test_all_32_views():
    """50 points matched between consecutive views only: every track is seen by all 32 views"""
    V, n, (H, W), cell = 32, 50, (48, 64), 4
    rng = np.random.default_rng(8)
    cells = np.stack([rng.permutation((H // cell) * (W // cell))[:n] for _ in range(V)])              # distinct cells per view
    px = np.stack([cells % (W // cell), cells // (W // cell)], -1) * cell + rng.uniform(0.25, 3.75, (V, n, 2))
    norm = np.stack([norm_px(px[..., 0], W), norm_px(px[..., 1], H)], -1)
    matches = np.concatenate([norm[:-1], norm[1:]], -1)
    certainty = rng.uniform(0.1, 1.0, (V - 1, n)).astype(np.float32)
    pairs, sizes = np.array([(v, v + 1) for v in range(V - 1)], np.int32), ((H, W),) * V
    got = _run(matches, certainty, pairs, sizes, cell=cell, max_tracks=64)
    _assert_equal(got, TR.build_tracks_ref(matches, certainty, pairs, sizes, cell=cell, max_tracks=64))
    assert tuple(got["counts"]) == (50, 0, 0, 0)
    assert (got["views"][:50] == -1).all() and (got["num_views"][:50] == 32).all() and got["visible"][:, :50].all()
    assert not got["views"][50:].any() and not got["visible"][:, 50:].any()


@pytest.mark.gpu
def test_unusable_matches_change_nothing_else():
    """Matches that are not usable for every reason there is, written over slots of the scene, against the same scene with those slots
    at certainty 0: the same tracks.  Both runs have the same usable matches, so no row moves."""
    inp = scene_inputs(5, 0)
    thresh = 0.25
    m, c = inp["matches"].copy(), inp["certainty"].copy()
    M, k = c.shape
    junk = np.zeros((M, k), bool)
    junk[:, 5::7] = True
    kinds = np.arange(M * k).reshape(M, k) % 5
    quiet = c.copy()
    quiet[junk] = 0.0
    m[junk & (kinds == 0)] = np.nan                                                     # NaN rows
    m[junk & (kinds == 1), 0] = 1.0                                                     # an endpoint at exactly x = 1.0
    c[junk & (kinds == 2)] = thresh
    c[junk & (kinds == 3)] = np.inf
    c[junk & (kinds == 4)] = np.nan
    mask = np.ones((M, k), np.uint8)
    mask.reshape(-1)[::3] = 0
    quiet[mask == 0] = 0.0
    # three more pairs that name no two different views, with the matches of pair 0
    extra = np.array([[2, 2], [-1, 1], [1, 5]], np.int32)
    m2, c2 = np.concatenate([m, np.repeat(inp["matches"][:1], 3, 0)]), np.concatenate([c, np.repeat(inp["certainty"][:1], 3, 0)])
    mask2, pairs2 = np.concatenate([mask, np.ones((3, k), np.uint8)]), np.concatenate([inp["pairs"], extra])
    got = _run(m2, c2, pairs2, inp["sizes"], mask=mask2, cell=4, certainty_thresh=thresh)
    _assert_equal(got, TR.build_tracks_ref(m2, c2, pairs2, inp["sizes"], mask=mask2, cell=4, certainty_thresh=thresh, max_tracks=T_FULL))
    base = _run(inp["matches"], quiet, inp["pairs"], inp["sizes"], cell=4, certainty_thresh=thresh)
    assert (got["track_of_match"][M:] == -1).all() and base["counts"][0] > 50
    got["track_of_match"] = got["track_of_match"][:M]
    _assert_equal(got, base)


@functools.lru_cache(maxsize=None)
def second_pass_inputs():
    """One pair, 300 matches.  View 0 is 1040 x 1024 at cell = 2: 266240 cells, 1040 blocks of 256, 16 more than the scan kernel's 1024
    threads take in one pass; a track's root is its cell in view 0 (the lowest id of the component), and 100 of the A ends lie in the
    last 16 pixel rows, which are the cells of blocks 1024 to 1039.  The B ends lie in distinct cells of a 64 x 64 view."""
    k, cell, sizes = 300, 2, ((1040, 1024), (64, 64))
    rng = np.random.default_rng(11)
    xa, ya = rng.uniform(0, 1024, k), np.concatenate([rng.uniform(0, 1024, 200), rng.uniform(1024, 1040, 100)])
    cb = rng.permutation(32 * 32)[:k]
    xb, yb = (cb % 32 + rng.uniform(0.1, 0.9, k)) * cell, (cb // 32 + rng.uniform(0.1, 0.9, k)) * cell
    matches = np.stack([norm_px(xa, 1024), norm_px(ya, 1040), norm_px(xb, 64), norm_px(yb, 64)], -1)[None]
    certainty = rng.uniform(0.1, 1.0, (1, k)).astype(np.float32)
    return _frozen(matches=matches, certainty=certainty, pairs=np.array([(0, 1)], np.int32), sizes=sizes), cell


@pytest.mark.gpu
def test_roots_beyond_the_first_pass_of_the_scan():
    """The scan of the per-block counts takes the blocks in passes of 1024: the ranks of the roots in blocks 1024 and above need the
    carry of the first pass."""
    inp, cell = second_pass_inputs()
    want = TR.build_tracks_ref(**inp, cell=cell, max_tracks=T_FULL)
    got = _run(**inp, cell=cell)
    _assert_equal(got, want)
    kept = int(got["counts"][0])
    assert 250 < kept <= 300
    # the rows ascend with the root's cell id: the last ones are the tracks of the last 16 pixel rows of view 0
    cells = (np.floor(got["x"][0, :kept, 1] / cell) * 512 + np.floor(got["x"][0, :kept, 0] / cell)).astype(np.int64)
    assert got["visible"][0, :kept].all() and (np.diff(cells) > 0).all()
    assert 80 < (cells >= 1024 * 256).sum() < kept - 80


@pytest.mark.gpu
def test_truncation_keeps_the_first_rows():
    full, want = scene_ref(5, 0), scene_ref(5, 0, 100)
    got = _run(**scene_inputs(5, 0), cell=4, max_tracks=100)
    _assert_equal(got, want)
    assert full["counts"][0] > 100 and np.array_equal(got["counts"], full["counts"])
    for name in ("views", "num_views"):
        assert np.array_equal(got[name], full[name][:100])
    assert np.array_equal(got["x"], full["x"][:, :100], equal_nan=True) and np.array_equal(got["visible"], full["visible"][:, :100])
    assert np.array_equal(got["track_of_match"], np.where(full["track_of_match"] < 100, full["track_of_match"], -1))


@pytest.mark.gpu
def test_run_to_run_and_graph_replay_are_bit_identical():
    from roma_amd import geometry
    inp = scene_inputs(5, 0)
    m, c, pairs = _dev(inp["matches"]), _dev(inp["certainty"]), _dev(inp["pairs"])

    def call():
        tr = geometry.build_tracks(m, c, pairs, inp["sizes"], cell=4, max_tracks=T_FULL)
        return tuple(getattr(tr, name) for name in FIELDS)

    def same(a, b):                                                  # bit patterns: x holds NaN
        return all(torch.equal(p.view(torch.uint8), q.view(torch.uint8)) for p, q in zip(a, b))

    first, second = call(), call()
    assert same(first, second) and int(first[5][3]) == 0 and int(first[5][0]) > 100
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
def test_tracks_feed_triangulate_nview():
    """Over the pure tracks, the median of |X^ - X| / |X - c0| from the tracks may exceed the median for the same points from the scene's
    own observations by at most 5 %: the two inputs differ by the fp32 round trip through normalised coordinates, a few 1e-4 px
    against 0.5 px of noise.  c0 is the mean camera centre."""
    from roma_amd import geometry
    s, inp = scene(5, 0), scene_inputs(5, 0)
    tr = geometry.build_tracks(_dev(inp["matches"]), _dev(inp["certainty"]), _dev(inp["pairs"]), inp["sizes"], cell=4, max_tracks=T_FULL)
    out = _fields(tr)
    R, t, K = _dev(s["R"]), _dev(s["t"]), _dev(s["K"])
    from_tracks = geometry.triangulate_nview(tr.x, R, t, K, visible=tr.visible)
    from_scene = geometry.triangulate_nview(_dev(s["x"]), R, t, K)
    pure = pure_tracks(out, s)
    rows, pts = np.array([r for r, _ in pure]), np.array([j for _, j in pure])
    assert len(pure) >= 0.9 * int((s["seen"].sum(0) >= 2).sum())
    c0 = np.mean([-s["R"][v].T @ s["t"][v] for v in range(5)], 0)
    X = s["X"][pts]
    err = lambda P: float(np.median(np.linalg.norm(P - X, axis=1) / np.linalg.norm(X - c0, axis=1)))
    e_tracks, e_scene = err(from_tracks.points.cpu().numpy()[rows].astype(np.float64)), err(from_scene.points.cpu().numpy()[pts].astype(np.float64))
    print(f"median relative error over {len(pure)} pure tracks: {e_tracks:.6f} from the tracks, {e_scene:.6f} from the scene's observations")
    assert e_tracks <= 1.05 * e_scene
