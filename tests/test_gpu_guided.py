"""Guided matching on the MI355X: sfd2_match_guided_batch and its Python layer against tests/guided_ref.py.  Comparisons are made on
SAFE rows (guided_ref.safe_rows: no pair of the row within BAND of the gate, its decisions further than the fp16 similarity error
EPS["f16"] = 1e-3 from changing): matches equal, scores within 5e-4, half of that error.  tests/test_guided_host.py asserts on the CPU
that at least 90 % of every scene's rows are safe and that the wrong variants used here change safe rows."""
import ctypes
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import guided_ref as gr
import match_ref as mr

pytestmark = pytest.mark.gpu

SCORE_TOL = 5e-4
KINDS = ["F", "H"]
EDGE_SIZES = [(0, 40), (40, 0), (1, 1), (1, 50), (50, 1)]


def _conf(c):
    return {"ratio_threshold": c["ratio"], "distance_threshold": c["dist"], "do_mutual_check": c["mutual"]}


def _problem(sc, t=None):
    p = (sc["d0"], sc["d1"], sc["xy0"], sc["xy1"], sc["kind"], sc["M"])
    return p if t is None else p + (t,)


def _run(scenes, conf, t=gr.MAX_ERROR):
    from sfd2_amd import two_view
    return two_view.guided_matches_batch([_problem(sc) for sc in scenes], t, _conf(conf))


def _compare(sc, conf, got, t=gr.MAX_ERROR, label=""):
    """The device's (matches0, scores0) of one pair against the restatement on its safe rows; returns the safe mask."""
    m, s = got
    n0 = len(sc["d0"])
    assert m.dtype == np.int64 and s.dtype == np.float32 and len(m) == len(s) == n0
    assert ((m >= -1) & (m < max(len(sc["d1"]), 1))).all() and np.isfinite(s).all()
    e, p = gr.gate64(sc["kind"], sc["M"], sc["xy0"], sc["xy1"], t)
    safe = gr.safe_rows(sc["sim"], e, t=t, **conf)
    rm, rs = gr.hloc_masked(sc["sim"], p, **conf)
    bad = np.flatnonzero(safe & (m != rm))
    assert bad.size == 0, f"{label}: rows {bad[:8]} got {m[bad[:8]]} want {rm[bad[:8]]}"
    err = np.abs(s.astype(np.float64) - rs)[safe]
    print(f"{label} {sc['kind']} {n0} x {len(sc['d1'])}: {int(safe.sum())} of {n0} rows safe, {int((rm >= 0).sum())} matched, "
          f"score error {err.max() if err.size else 0.0:.2e}")
    assert (err <= SCORE_TOL).all()
    assert ((m[~p.any(axis=1) & safe] == -1)).all() and not s[~p.any(axis=1) & safe].any()
    return safe


def _same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


@pytest.mark.parametrize("conf", list(gr.CONFS))
@pytest.mark.parametrize("kind", KINDS)
def test_sizes_in_one_batch_alone_and_twice(kind, conf):
    """Sub-tile, stage, query-block and split seams in one batch with empty and one-point pairs; each pair alone and every run twice
    give the batch's bytes."""
    c = gr.CONFS[conf]
    scenes = [gr.scene(kind, n0, n1) for n0, n1 in gr.SIZES[:3] + EDGE_SIZES[:2] + gr.SIZES[3:] + EDGE_SIZES[2:]]
    batch = _run(scenes, c)
    again = _run(scenes, c)
    assert len(batch) == len(scenes)
    compared = 0
    for sc, got, got2 in zip(scenes, batch, again):
        assert _same(got, got2)
        compared += int(_compare(sc, c, got, label=conf).sum())
        alone = _run([sc], c)[0]
        assert _same(alone, got) and _same(alone, _run([sc], c)[0])
    assert compared > 2000
    for sc, got in zip(scenes, batch):
        if len(sc["d0"]) == 0 or len(sc["d1"]) == 0:
            assert len(got[0]) == len(sc["d0"]) and (got[0] == -1).all() and not got[1].any()


@pytest.mark.parametrize("kind", KINDS)
def test_twin_scene_gate_is_applied_per_element(kind):
    sc = gr.twin_scene(kind=kind)
    c = gr.CONFS["RATIO"]
    got = _run([sc], c)[0]
    safe = _compare(sc, c, got, label="twin")
    w, _ = gr.hloc_no_gate(sc["sim"], **c)
    changed = (got[0] != w)[safe].mean()
    print(f"twin scene {kind}: the device keeps {(got[0] >= 0).sum()}, the rule without the gate {(w >= 0).sum()}; {changed:.2f} of the safe rows differ")
    assert changed >= 0.2
    tw = sc["twinned"][safe[sc["twinned"]]]
    assert (got[0][tw] >= 0).mean() > 0.9               # the rows whose look-alike wins or spoils the ratio without the gate


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [(300, 300), (300, 2049)])
def test_forced_positions(kind, n):
    """A better-scoring candidate just outside the gate (>= 10 BAND) in the same register, the neighbouring register, the other
    half-wave, the other sub-tile and either side of a split boundary relative to the gated best: the gated best wins."""
    n0, n1 = n
    chunk, pairs = gr.forced_pairs(n1)
    assert gr.splits(1, max(n0, n1)) == 8 and chunk == gr.chunk(n1, 8)
    sc = gr.forced_scene(kind, n0, n1, pairs)
    for name, c in gr.CONFS.items():
        got = _run([sc], c)[0]
        safe = _compare(sc, c, got, label="forced " + name)
        assert safe[sc["q"]].all() and (got[0][sc["q"]] == sc["j1"]).all()
        assert np.abs(got[1][sc["q"]] - (sc["sim"][sc["q"], sc["j1"]] + 1) / 2).max() <= SCORE_TOL
    if kind == "F":     # the same placements as CANDIDATES OF THE REVERSE SWEEP: images swapped, x0^T F^T x1 = 0
        sw = dict(kind="F", M=np.ascontiguousarray(sc["M"].T), d0=sc["d1"], d1=sc["d0"], xy0=sc["xy1"], xy1=sc["xy0"], sim=np.ascontiguousarray(sc["sim"].T))
        for name in ("NNM", "RATIO"):
            got = _run([sw], gr.CONFS[name])[0]
            safe = _compare(sw, gr.CONFS[name], got, label="forced swapped " + name)
            assert safe[sc["j1"]].all() and (got[0][sc["j1"]] == sc["q"]).all() and (got[0][sc["j2"]] != sc["q"]).all()


def _writable(sc):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}


@pytest.mark.parametrize("mutual", [False, True])
def test_rows_and_columns_without_a_gated_candidate(mutual):
    """Row 0 and column 0 both empty, their descriptors equal (the best similarity of both): -1 and score 0, with and without the mutual
    check and without a distance threshold -- the case the unguarded decision would match."""
    sc = _writable(gr.scene("H", 257, 300))
    sc["xy0"][0] = (9.0e4, 9.0e4)
    sc["xy1"][0] = (-9.0e4, 7.0e4)
    sc["d1"][0] = sc["d0"][0]
    sc["sim"] = mr.similarity(sc["d0"], sc["d1"])
    _, p = gr.gate64("H", sc["M"], sc["xy0"], sc["xy1"])
    assert not p[0].any() and not p[:, 0].any() and np.argmax(sc["sim"][0]) == 0
    empty = np.flatnonzero(~p.any(axis=1))
    assert len(empty) > 10
    for ratio in (None, 0.8):
        c = dict(ratio=ratio, dist=None, mutual=mutual)
        m, s = _run([sc], c)[0]
        _compare(sc, c, (m, s), label="empty rows")
        assert (m[empty] == -1).all() and not s[empty].any() and m[0] == -1 and s[0] == 0 and not (m == 0).any()
        # a gate nothing passes: every row empty
        m, s = _run([sc], c, t=1e-4)[0]
        assert not gr.gate64("H", sc["M"], sc["xy0"], sc["xy1"], 1e-4)[1].any() and (m == -1).all() and not s.any()


def test_rows_with_exactly_one_gated_candidate():
    """s2 = -inf: the ratio test passes whatever the ratio (the existing one-candidate rule)."""
    sc = gr.scene("H", 700, 2049)
    e, p = gr.gate64("H", sc["M"], sc["xy0"], sc["xy1"])
    c = dict(ratio=0.3, dist=None, mutual=False)
    m, s = _run([sc], c)[0]
    safe = _compare(sc, c, (m, s), label="one candidate")
    one = np.flatnonzero((p.sum(axis=1) == 1) & safe)
    assert len(one) > 100 and (m[one] == np.argmax(p[one], axis=1)).all() and (s[one] > 0).all()
    c = dict(ratio=0.3, dist=None, mutual=True)
    m, s = _run([sc], c)[0]
    safe = _compare(sc, c, (m, s), label="one candidate, mutual")
    both = np.flatnonzero((p.sum(axis=1) == 1) & safe & (p.sum(axis=0)[np.argmax(p, axis=1)] == 1))     # alone in its row AND its column
    assert len(both) > 100 and (m[both] == np.argmax(p[both], axis=1)).all()


def test_bit_equal_duplicates_inside_the_gate():
    """The first index wins and no ratio below 1 passes; a duplicate OUTSIDE the gate does not count."""
    sc = _writable(gr.scene("F", 257, 300))
    rows, cols = sc["rows"][:40], sc["cols"][:40]
    free = np.setdiff1d(np.arange(300), sc["cols"])[:40]
    for j, f in zip(cols[:20], free[:20]):                # inside: same descriptor, same place
        sc["d1"][f], sc["xy1"][f] = sc["d1"][j], sc["xy1"][j]
    for j, f in zip(cols[20:], free[20:]):                # outside: same descriptor, 300 px off the epipolar line
        i = rows[20:][list(cols[20:]).index(j)]
        l = sc["M"] @ np.array([sc["xy0"][i, 0], sc["xy0"][i, 1], 1.0])
        sc["d1"][f], sc["xy1"][f] = sc["d1"][j], sc["xy1"][j] + 300.0 * l[:2] / np.linalg.norm(l[:2])
    sc["sim"] = mr.similarity(sc["d0"], sc["d1"])
    e, p = gr.gate64("F", sc["M"], sc["xy0"], sc["xy1"])
    assert p[rows[:20], free[:20]].all() and p[rows, cols].all() and not p[rows[20:], free[20:]].any()
    assert (sc["sim"][rows, cols] == sc["sim"][rows, free]).all() and (sc["sim"][rows, cols] > 0.69).all()
    m, _ = _run([sc], dict(ratio=None, dist=None, mutual=False))[0]
    assert (m[rows[:20]] == np.minimum(cols[:20], free[:20])).all() and (m[rows[20:]] == cols[20:]).all()
    m, _ = _run([sc], dict(ratio=0.999, dist=None, mutual=False))[0]
    assert (m[rows[:20]] == -1).all() and (m[rows[20:]] == cols[20:]).all()
    rm, _ = gr.hloc_masked(sc["sim"], p, ratio=0.999, mutual=False)
    assert (rm[rows[:20]] == -1).all() and (rm[rows[20:]] == cols[20:]).all()


@pytest.mark.parametrize("name", ["NNM", "RATIO"])
def test_a_gate_that_passes_everything_is_the_plain_matcher(name):
    from sfd2_amd import _lib
    sc = gr.scene("F", 700, 2049)
    c = gr.CONFS[name]
    assert gr.gate64("F", sc["M"], sc["xy0"], sc["xy1"], 1e6)[1].all() and gr.gate32("F", sc["M"], sc["xy0"], sc["xy1"], 1e6)[1].all()
    m, s = _run([sc], c, t=1e6)[0]
    ctx = _lib.default_context(0)
    mc = _lib.MatchConf(_lib.MATCH_HLOC, int(c["mutual"]), float(c["ratio"] or 0.0), float(c["dist"] or 0.0), _lib.SIM_F16)
    pm, ps = np.empty(700, dtype=np.int64), np.empty(700, dtype=np.float32)
    _lib.check(ctx.lib.sfd2_match(ctx.h, sc["d0"].ctypes.data, 700, sc["d1"].ctypes.data, 2049, 128, _lib.DT_F32, _lib.LAYOUT_ND, 0, ctypes.byref(mc),
                                  pm.ctypes.data, ps.ctypes.data, 0))
    safe = mr.margins(None, None, "hloc", c["ratio"], c["dist"], c["mutual"], eps=1e-3, sim=sc["sim"])
    print(f"{name}: {int(safe.sum())} of 700 rows safe; matches byte-equal {m.tobytes() == pm.tobytes()}, scores byte-equal {s.tobytes() == ps.tobytes()}, "
          f"largest score difference {np.abs(s - ps).max():.3e}")
    assert safe.mean() > 0.9 and (m[safe] == pm[safe]).all() and np.abs(s - ps)[safe].max() <= 2.0 ** -20


def _raw(problems, conf, n_out):
    from sfd2_amd import _lib
    ctx = _lib.default_context(0)
    m, s = np.full(max(n_out, 1), -7, dtype=np.int64), np.full(max(n_out, 1), -7, dtype=np.float32)
    rc = ctx.lib.sfd2_match_guided_batch(ctx.h, (_lib.GuidedProblem * len(problems))(*problems), len(problems), 128, ctypes.byref(conf), m.ctypes.data,
                                         s.ctypes.data, 0)
    return rc, m[:n_out], s[:n_out], ctx.lib.sfd2_last_error().decode()


def _raw_problem(sc, keep, t=gr.MAX_ERROR):
    from sfd2_amd import _lib
    pr = _lib.GuidedProblem()
    for dst, d in ((pr.d0, sc["d0"]), (pr.d1, sc["d1"])):
        d = np.ascontiguousarray(d, dtype=np.float32)
        keep.append(d)
        dst.data, dst.n, dst.dtype, dst.layout, dst.on_device, dst.rows, dst.n_rows = d.ctypes.data, len(d), _lib.DT_F32, _lib.LAYOUT_ND, 0, None, 0
    k0, k1 = np.ascontiguousarray(sc["xy0"], dtype=np.float32), np.ascontiguousarray(sc["xy1"], dtype=np.float32)
    keep += [k0, k1]
    pr.xy0, pr.xy1, pr.model, pr.max_error_px = k0.ctypes.data, k1.ctypes.data, (_lib.GUIDE_F if sc["kind"] == "F" else _lib.GUIDE_H), t
    for j in range(9):
        pr.M[j] = np.asarray(sc["M"]).reshape(-1)[j]
    return pr


def test_device_resident_packed_sets_give_the_host_bytes():
    import torch
    from sfd2_amd import _lib
    scenes = [gr.scene("F", 257, 300), gr.scene("H", 300, 257)]
    c = gr.CONFS["RATIO"]
    host = _run(scenes, c)
    ctx = _lib.default_context(0)
    keep, probs = [], []
    for sc in scenes:
        pr = _raw_problem(sc, keep)
        for dst in (pr.d0, pr.d1):
            packed = torch.empty((dst.n, 128), dtype=torch.float16, device="cuda:0")
            _lib.check(ctx.lib.sfd2_desc_pack(ctx.h, ctypes.byref(dst), 128, packed.data_ptr(), 0))
            keep.append(packed)
            dst.data, dst.dtype, dst.on_device = packed.data_ptr(), _lib.DT_F16, 1
        probs.append(pr)
    mc = _lib.MatchConf(_lib.MATCH_HLOC, 1, 0.8, 0.0, _lib.SIM_F16)
    rc, m, s, err = _raw(probs, mc, 257 + 300)
    assert rc == 0, err
    assert m.tobytes() == np.concatenate([h[0] for h in host]).tobytes() and s.tobytes() == np.concatenate([h[1] for h in host]).tobytes()


def test_projection_that_is_not_finite():
    """H (x0, y0, 1) with a zero third coordinate: the record says invalid, the row gets -1."""
    sc = _writable(gr.scene("H", 257, 300))
    sc["M"] = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 0.0, -100.0]])
    bad = np.arange(0, 257, 9)
    sc["xy0"][bad, 0] = 100.0
    sc["xy0"][bad[:3]] = (100.0, 0.0)                                                   # 0 / 0 too
    sc["xy0"][bad[3], 0] = 0.0                                                           # ... and 0 / -100: fine
    with np.errstate(divide="ignore", invalid="ignore"):
        proj = sc["xy0"][:200] / (sc["xy0"][:200, 0:1] - 100.0) + 0.25                  # the projections of the first 200 rows
    sc["xy1"][:200] = np.where(np.isfinite(proj), proj, 50.0)
    assert np.isfinite(sc["xy1"]).all()
    e, p = gr.gate64("H", sc["M"], sc["xy0"], sc["xy1"])
    dead = np.setdiff1d(bad, bad[3:4])
    assert np.isinf(e[dead]).all() and p[np.setdiff1d(np.arange(200), dead), np.setdiff1d(np.arange(200), dead)].all()
    for c in gr.CONFS.values():
        m, s = _run([sc], c)[0]
        _compare(sc, c, (m, s), label="invalid projection")
        assert (m[dead] == -1).all() and not s[dead].any() and (m >= 0).sum() > 50


def test_error_returns_name_the_pair_and_the_field():
    from sfd2_amd import _lib
    sc = gr.scene("F", 65, 64)
    ok = _lib.MatchConf(_lib.MATCH_HLOC, 1, 0.0, 0.0, _lib.SIM_F16)
    keep = []

    def two(change):
        probs = [_raw_problem(sc, keep), _raw_problem(sc, keep)]
        change(probs[1])
        return probs

    rows = np.arange(4, dtype=np.int32)
    xy_nan = np.array(sc["xy1"], dtype=np.float32)
    xy_nan[5, 1] = np.nan
    cases = [(lambda p: setattr(p, "model", 7), ok, "problem 1: model"),
             (lambda p: setattr(p.d0, "rows", rows.ctypes.data), ok, "problem 1: d0.rows must be NULL"),
             (lambda p: setattr(p.d1, "rows", rows.ctypes.data), ok, "problem 1: d1.rows must be NULL"),
             (lambda p: setattr(p, "xy1", xy_nan.ctypes.data), ok, "problem 1: non-finite xy1"),
             (lambda p: p.M.__setitem__(4, float("inf")), ok, "problem 1: non-finite M"),
             (lambda p: setattr(p, "max_error_px", 0.0), ok, "problem 1: max_error_px"),
             (lambda p: setattr(p, "max_error_px", float("nan")), ok, "problem 1: max_error_px"),
             (lambda p: None, _lib.MatchConf(_lib.MATCH_ITLOC_NNM, 1, 0.0, 0.0, _lib.SIM_F16), "conf.flavour"),
             (lambda p: None, _lib.MatchConf(_lib.MATCH_ITLOC_NNR, 1, 0.9, 0.0, _lib.SIM_F16), "conf.flavour"),
             (lambda p: None, _lib.MatchConf(_lib.MATCH_HLOC, 1, 0.0, 0.0, _lib.SIM_F16X2), "conf.sim_mode")]
    for change, conf, text in cases:
        rc, m, s, err = _raw(two(change), conf, 130)
        assert rc == -1 and text in err and "sfd2_match_guided_batch" in err, (text, err)
        assert (m == -7).all() and (s == -7).all()              # nothing written
    rc, m, s, err = _raw(two(lambda p: None), ok, 130)
    assert rc == 0 and m[:65].tobytes() == m[65:].tobytes()


# ---------------------------------------------------------------------------------------------------------------- the command
def _store_scene(root):
    """Three images of tri_ref's scene with descriptors: one per track of the true matches (cosine 0.9 to the track's own), random for
    the rest; matches0 of the plain matcher's kind (the scene's matches, a tenth of them wrong)."""
    import tri_ref
    from sfd2_amd import colmap_io, feature_io, synth
    from sfd2_amd.match_features import names_to_pair
    sc = tri_ref.make_scene(seed=5, n_images=3, n_points=80, n_clutter=12, window=3, n_joiners=0, n_weak_pairs=0, p_visible=0.9, noise_px=0.5, spacing=1.5)
    rs = np.random.RandomState(11)
    ids = sorted(sc["keypoints"])
    base = {i: synth.make_descriptors(len(sc["keypoints"][i]), seed=60 + i).astype(np.float64) for i in ids}
    for i0, i1, m in sc["pair_matches"]:                  # chain the descriptors along the matches, in pair order
        base[i1][m[:, 1]] = mr._at_cosine(base[i0][m[:, 0]], np.full(len(m), 0.9), rs)
    desc = {i: mr._fp16(base[i]) for i in ids}
    name = {i: im.name for i, im in sc["images"].items()}
    ref = root / "ref"
    empty = {i: colmap_io.Image(i, im.qvec, im.tvec, im.camera_id, im.name, np.zeros((0, 2)), np.zeros(0, np.int64)) for i, im in sc["images"].items()}
    colmap_io.write_model(sc["cameras"], empty, {}, ref)
    (root / "pairs.txt").write_text("\n".join(f"{name[a]} {name[b]}" for a, b in sc["pairs"]) + "\n")
    feats = feature_io.open_store(str(root / "feats.h5"), "a")
    for i in ids:
        kp = sc["keypoints"][i]
        feature_io.write_features(feats, name[i], {"keypoints": kp.astype(np.float64), "descriptors": desc[i].T.astype(np.float64), "scores": np.ones(len(kp)),
                                                   "image_size": np.array([640, 480])})
    feats.close()
    store = feature_io.open_store(str(root / "matches.h5"), "a")
    for i0, i1, m in sc["pair_matches"]:
        m0 = np.full(len(sc["keypoints"][i0]), -1, dtype=np.int64)
        m0[m[:, 0]] = m[:, 1]
        feature_io.write_matches(store, names_to_pair(name[i0], name[i1]), m0, np.where(m0 >= 0, 0.9, 0.0).astype(np.float32))
    store.close()
    return sc, desc, name, ref


def _groups(path):
    from sfd2_amd import feature_io
    st = feature_io.open_store(str(path), "r")
    out = {k: {d: np.asarray(st[k][d].__array__()) for d in st[k].keys()} for k in st.keys()}
    st.close()
    return out


def test_command_end_to_end(tmp_path):
    from sfd2_amd import geometric_verification as gv, triangulation, two_view
    from sfd2_amd.match_features import confs, names_to_pair
    sc, desc, name, ref = _store_scene(tmp_path)
    pairs, feats, matches = tmp_path / "pairs.txt", tmp_path / "feats.h5", tmp_path / "matches.h5"
    src = _groups(matches)
    # without the flag: today's output -- the input's groups with the entries outside the kept mask set to -1 -- whether the option is left out or False
    res = gv.main(pairs, feats, matches, tmp_path / "plain.h5", reference_sfm_model=ref, model="geometry")
    res_f = gv.main(pairs, feats, matches, tmp_path / "plain_false.h5", reference_sfm_model=ref, model="geometry", guided_matching=False)
    plain = _groups(tmp_path / "plain.h5")
    assert open(tmp_path / "plain.h5", "rb").read() == open(tmp_path / "plain_false.h5", "rb").read()
    for i0, i1, m in sc["pair_matches"]:
        g0, g1, r = src[names_to_pair(name[i0], name[i1])], plain[names_to_pair(name[i0], name[i1])], res[name[i0], name[i1]]
        assert np.array_equal(r["inliers"], res_f[name[i0], name[i1]]["inliers"]) and r["num_inliers"] >= 15
        want, rows = np.full_like(g0["matches0"], -1), np.flatnonzero(g0["matches0"] >= 0)      # the mask runs over the matched rows in order
        want[rows[r["inliers"]]] = g0["matches0"][rows[r["inliers"]]]
        assert set(g1) == set(g0) and g1["matches0"].dtype == g0["matches0"].dtype and np.array_equal(g1["matches0"], want)
        assert g1["matching_scores0"].tobytes() == g0["matching_scores0"].tobytes()
    # with it: the groups are guided_match_pairs' on the same inputs
    res_g = gv.main(pairs, feats, matches, tmp_path / "guided.h5", reference_sfm_model=ref, model="geometry", guided_matching=True, guided_conf="NNM")
    guided = _groups(tmp_path / "guided.h5")
    ids = {n: i for i, n in name.items()}
    order = [(ids[a], ids[b]) for a, b in (ln.split() for ln in pairs.read_text().splitlines())]
    pm = [(a, b, next(m for i0, i1, m in sc["pair_matches"] if (i0, i1) == (a, b))) for a, b in order]
    results = [res_g[name[a], name[b]] for a, b in order]
    kps = {i: sc["keypoints"][i].astype(np.float32) for i in name}
    cams = {i: sc["cameras"][sc["images"][i].camera_id] for i in name}
    ims = {i: type("Im", (), {"camera_id": i})() for i in name}
    gm, off, counts, gs = two_view.guided_match_pairs(kps, desc, pm, results, 4.0, confs["NNM"], cams, ims)
    more = 0
    for p, (a, b) in enumerate(order):
        g0, g1 = src[names_to_pair(name[a], name[b])], guided[names_to_pair(name[a], name[b])]
        assert set(g1) == set(g0) and g1["matches0"].dtype == g0["matches0"].dtype and g1["matches0"].shape == g0["matches0"].shape
        assert g1["matching_scores0"].dtype == g0["matching_scores0"].dtype and g1["matching_scores0"].shape == g0["matching_scores0"].shape
        assert np.array_equal(g1["matches0"].reshape(-1), gm[off[p]:off[p + 1], 1].astype(g0["matches0"].dtype))
        assert np.array_equal(g1["matching_scores0"].reshape(-1), gs[off[p]:off[p + 1]].astype(g0["matching_scores0"].dtype))
        assert counts[p] == (g1["matches0"] >= 0).sum() >= 15
        more += int((g1["matches0"] >= 0).sum()) - int((plain[names_to_pair(name[a], name[b])]["matches0"] >= 0).sum())
    print(f"guided matching keeps {more:+d} matches over verification alone on {len(order)} pairs")
    # the readers of `triangulation --skip_geometric_verification` open it
    kp_read, pm_read = triangulation.read_inputs(sc["images"], pairs, feats, tmp_path / "guided.h5")
    assert len(pm_read) == len(order) and all(len(m) == counts[p] for p, (_, _, m) in enumerate(pm_read))
    # the command line writes the same file, with another rule too
    subprocess.run([sys.executable, "-m", "sfd2_amd.geometric_verification", "--pairs", str(pairs), "--features", str(feats), "--matches", str(matches),
                    "--output", str(tmp_path / "cli.h5"), "--reference_sfm_model", str(ref), "--model", "geometry", "--guided_matching"],
                   check=True, timeout=120, cwd=str(Path(__file__).resolve().parent.parent))
    cli = _groups(tmp_path / "cli.h5")
    assert set(cli) == set(guided) and all(np.array_equal(cli[k][d], guided[k][d]) for k in guided for d in guided[k])


@pytest.mark.parametrize("model", ["essential", "fundamental"])
def test_command_with_the_other_models(tmp_path, model):
    from sfd2_amd import geometric_verification as gv
    from sfd2_amd.match_features import names_to_pair
    sc, desc, name, ref = _store_scene(tmp_path)
    kw = dict(reference_sfm_model=ref) if model == "essential" else {}
    gv.main(tmp_path / "pairs.txt", tmp_path / "feats.h5", tmp_path / "matches.h5", tmp_path / "g.h5", model=model, guided_matching=True, guided_conf="NNR", **kw)
    out, src = _groups(tmp_path / "g.h5"), _groups(tmp_path / "matches.h5")
    for i0, i1, m in sc["pair_matches"]:
        g, g0 = out[names_to_pair(name[i0], name[i1])], src[names_to_pair(name[i0], name[i1])]
        true = g0["matches0"].reshape(-1)
        kept = g["matches0"].reshape(-1)
        assert kept.dtype == true.dtype and (kept >= 0).sum() >= 15
        agree = (kept == true)[(kept >= 0) & (true >= 0)].mean()
        print(model, name[i0], name[i1], f"{(kept >= 0).sum()} guided matches, {agree:.2f} of those the input also matched agree with it")
        assert agree > 0.8
