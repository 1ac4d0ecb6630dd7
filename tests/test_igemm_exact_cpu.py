"""The case tables and references of tests/test_igemm_exact_gpu.py, checked without a GPU: every run reaches the route, fast flag and
split count it names (pt_igemm_plan under the same hooks - host only); a mirror of tail_variant() shows that every (pipelined kernel,
tail variant) pair and every plain-loop route is reached; every table entry meets its preconditions on its fp64 reference; pt_gelu_erf's
formula in numpy fp32 gives max(g, 0) - up to the signed-zero product - for every gate value that occurs; and recipe() - the kernel's
index arithmetic (row_origin, tap_source, walk_step, class_of / out_row, vec_index) in torch fp32 - reproduces fp64 F.conv2d / F.conv3d
for every gather case, while each planted break changes at least one output of the case that names it: "the GPU test would fail if
the kernel were subtly wrong" is itself tested here."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_igemm_exact_gpu as G

name_of = lambda c: c.name


# ------------------------------------------------------------------------------------------------- the tables
def test_every_run_reaches_the_plan_it_names():
    """cfg and split count from the library's planner; the fast flag from forced cfg 3, which the planner keeps only for channel-aligned K
    (igemm.hip:942); the rasterisation group of the tuned case."""
    for c, force, cfg_named, offer_ws in G.all_runs():
        cfg, splits, gm, need = G.planned(c, force, offer_ws)
        if cfg_named is not None:
            assert cfg == cfg_named, (c.name, force, cfg)
        assert splits == (c.splits if offer_ws else 1), (c.name, force, splits)
        assert (need > 0) == (c.splits > 1 and force in (-1, 3)), (c.name, force, need)
        if offer_ws:
            g = G.geometry(c)
            assert need == c.splits * g["M"] * g["N"] * 4
    for c in G.ALL_CASES:
        assert (G.planned(c, 3, False)[0] == 3) == G.is_fast(c), c.name
    c = G.CASES["lin_group"]
    for force in (0, 3, 5):                                       # six M tiles of 256 in groups of 4: the second group has gm = 2; the grid is no multiple of 8
        cfg, _, gm, _ = G.planned(c, force, False)
        tiles_m, tiles_n = -(-1320 // G.BM[cfg]), -(-640 // G.BN[cfg])
        assert gm == 4 and tiles_m == 6 and tiles_m % gm == 2
    assert (6 * 3) % 8 != 0 and (6 * 2) % 8 != 0                  # cfg 0 and cfg 3 (pt_xcd_remap)


def test_split_ranges():
    """igemm.hip:500-503: ceil(nk / splits) K tiles per split - the linear case ends on a split of one tile, the convolution splits evenly."""
    for c, ranges in ((G.CASES["splitk_lin_bias"], (7,) * 7 + (1,)), (G.CASES["splitk_conv_bias"], (6,) * 9)):
        nk = G.geometry(c)["K"] // G.BK
        per = -(-nk // c.splits)
        assert tuple(min(per, nk - s * per) for s in range(c.splits)) == ranges


def test_every_kernel_instance_is_reached():
    """launch_pipelined's table (igemm.hip:814-818) and the plain-loop launches (:1010-1014), by the mirror of tail_variant()."""
    pipelined, plain = set(), set()
    for c, force, cfg_named, offer_ws in G.all_runs():
        cfg, splits, _, _ = G.planned(c, force, offer_ws)
        fast = G.is_fast(c)
        if splits > 1:
            pipelined.add((3, "SPLITK"))
        elif cfg == 3 or (cfg == 0 and fast):
            pipelined.add((cfg, c.variant))
        else:
            plain.add(G.route_name(cfg, fast))
    variants = {"P0", "P1", "P2", "EW", "W0", "W1", "W2", "G0", "GEW"}
    assert pipelined == {(k, v) for k in (0, 3) for v in variants} | {(3, "SPLITK")}
    assert plain == {"cfg0g", "cfg1f", "cfg1g", "cfg2f", "cfg2g", "cfg4f", "cfg4g", "cfg5f", "cfg5g"}
    for shape in G.TAIL_SHAPES:                                   # every variant on both tail shapes, on both pipelined kernels and cfg 1, 2, 4, 5
        seen = {c.variant: {f for f, _ in c.routes} for c in G.TAIL_CASES if f"_{shape}_" in c.name}
        assert set(seen) == variants
        assert all(r >= ({0, 2, 3, 4} if v in ("G0", "GEW") else {0, 1, 2, 3, 4, 5}) for v, r in seen.items())


def wave_paths(cfg, n_out):
    """Per workgroup column (N tile) the set of tail paths its waves take: "fast" (whole wave), "ew" (ragged: igemm_tail.h:192), "past"."""
    tiles = []
    for n0 in range(0, n_out, G.BN[cfg]):
        waves = range(n0, n0 + G.BN[cfg], G.WAVE_W[cfg])
        tiles.append({"fast" if w + G.WAVE_W[cfg] <= n_out else ("ew" if w < n_out else "past") for w in waves})
    return tiles


def test_the_mixed_shape_mixes_the_tails_in_one_workgroup():
    assert wave_paths(3, 400)[1] == {"ew", "past"} and wave_paths(3, 400)[0] == {"fast"}        # 320-wide tile: wave 0 ragged, wave 1 past N
    assert wave_paths(0, 400)[1] == {"fast", "ew"}                                              # 256-wide tile: a whole and a ragged 128-wide wave
    assert wave_paths(1, 400)[1] == {"fast", "past"} and wave_paths(4, 400)[2] == {"ew"} and wave_paths(2, 400)[3] == {"ew", "past"}
    for cfg in range(6):
        assert all(t == {"fast"} for t in wave_paths(cfg, 640)) or cfg == 0                     # (600, 640): whole waves everywhere ...
    assert wave_paths(0, 640)[2] == {"fast", "past"}                                            # ... but for the wave beyond N on the 256-wide tile


# ------------------------------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("c", G.ALL_CASES, ids=name_of)
def test_preconditions(c):
    """problem() asserts them: integer partial sums below 2^24, the epilogue chain equal in fp32 and fp64 at every step, |out| < 60000,
    a saturated gate.  Here also: what the comments of the tables promise about the data."""
    pr = G.problem(c)
    g = pr["geo"]
    assert pr["out"].shape == (g["M"], g["n_out"]) and bool(torch.isfinite(pr["out"].float()).all())
    assert pr["out"].dtype == (torch.float32 if c.out_f32 else torch.float16)
    if c.out_lo:                                                  # the low half is worth checking: a good part of it is no zero
        assert int((pr["out_lo"] != 0).sum()) > pr["out_lo"].numel() // 4
    if c.res_lo:
        assert sorted(set(pr["res_lo"].flatten().tolist())) == [-0.5, -0.25, 0.25, 0.5]
    if c.vec == 2:                                                # the index wraps
        raw = G.vec_rows(c, g["M"], broken="vec_mod")
        assert int(raw.max()) >= G.VB and int(G.vec_rows(c, g["M"]).max()) == G.VB - 1
    if c.vec == 1:
        assert 256 % G.VG and 16 % G.VG and g["M"] > G.VG
    if c.kind == "fold":                                          # folded weights: sums of at most four integers
        w = pr["pack"].w.float()
        assert bool((w == w.round()).all()) and float(w.abs().max()) <= 8 and w.shape[0] == 4 * 384
    if c.name == "c3_1x1_images":                                 # eight taps fully masked: the result is the centre tap alone
        centre = pr["x0"].double() @ pr["pack"].w[:64, 4 * 64:5 * 64].double().t() + pr["pack"].bias[:64].double()
        assert torch.equal(centre, pr["t64"])
    if c.name == "wide_image":
        assert g["Wout"] == 1200 and g["Hout"] == 2 and not G.is_fast(c)


def test_out_rounds_once():
    """What the kernel's fp32 -> fp16 conversion gives is .half() of the fp64 value: both round the same exact value once (ties included)."""
    n = torch.arange(-(2 ** 20), 2 ** 20, 3, dtype=torch.float64)
    for s in (2.0 ** -5, 0.5, 0.125, 2.0):
        v = n * s
        v = v[v.abs() < 60000]
        assert torch.equal(v.half(), v.float().half())


# ------------------------------------------------------------------------------------------------- the saturated gate
def gelu_erf_f32(x):
    """pt_gelu_erf (pt_common.h:67-77) in numpy fp32, operation by operation; exp2 through fp64 and rounded (the device's v_exp_f32 is
    accurate to an ulp: the argument below does not depend on the last bits of a number below 2^-50)."""
    f = np.float32
    x = x.astype(f)
    ax = np.abs(x)
    z = ax * f(0.70710678118654752)
    q = np.full_like(z, f(0.00294415708))
    for coef in (-0.0295900398, 0.148665627, 0.918509366, 1.62788901):
        q = q * z + f(coef)
    e = np.exp2(-(q * z).astype(np.float64)).astype(f)
    return (x + ax) * f(0.5) - f(0.5) * ax * e, q * z


def test_gelu_is_saturated_at_every_gate_value_that_occurs():
    """For every gate value of every GEGLU case: the formula gives g exactly for g > 0 and for g < 0 a value in (-2^-50 |g|, 0] whose
    product with any |value| < 2^24, times out_scale, rounds to a signed zero in fp16.  This rests on the fit's coefficients as
    committed in pt_common.h: if they change, this test is what says so."""
    cases = [c for c in G.ALL_CASES if c.geglu]
    assert len(cases) >= 5
    gates = np.unique(np.concatenate([G.problem(c)["gate"].numpy().ravel() for c in cases] + [np.array([8.0, -8.0])]))
    assert np.abs(gates).min() == 8 and np.all(gates % 16 == 8)
    y, qz = gelu_erf_f32(gates)
    assert qz[np.abs(gates) == 8].min() > 52 and np.all(np.diff(qz[gates > 0]) > 0)               # q z ~ 52.3 at |g| = 8 and increasing
    pos = gates > 0
    assert np.array_equal(y[pos], gates[pos].astype(np.float32))
    neg = y[~pos]
    assert np.all(neg <= 0) and np.all(-neg < np.abs(gates[~pos]) * 2.0 ** -50)
    worst = neg.astype(np.float64) * 2.0 ** 24 * max(c.out_scale for c in cases)                 # the largest product any case can form
    assert np.all(worst.astype(np.float16) == 0)
    for c in cases:                                               # and so the reference is val * max(g, 0)
        pr = G.problem(c)
        n = pr["geo"]["n_out"]
        val, g32 = pr["t64"][:, :n].numpy().astype(np.float32), pr["gate"].numpy()
        act = gelu_erf_f32(g32)[0]
        got = torch.from_numpy((val * act * np.float32(c.out_scale)).astype(np.float32))
        if c.res:
            got = (torch.from_numpy(val * act) + pr["res"].float()) * c.out_scale
        assert torch.equal(G.positive_zero(got.half()), G.positive_zero(pr["out"]))


# ------------------------------------------------------------------------------------------------- the kernel's index arithmetic
GATHERED = [c for c in G.ALL_CASES if c.kind != "lin"]


@pytest.mark.parametrize("c", GATHERED, ids=name_of)
def test_the_kernels_index_arithmetic_gives_the_fp64_convolution(c):
    got = G.recipe(c)
    assert got.dtype == torch.float32 and torch.equal(got.double(), G.problem(c)["t64"])


# (break, the case that names it)
BREAKS = [("bounds", "c3_2x7x5"), ("bounds", "c3_3x19x23"), ("bounds", "up1_c64"), ("bounds_left", "wide_image"), ("bounds_left", "c3_2x7x5"), ("bounds", "c3_downsample"),
          ("parity", "fold_3x9x7"), ("parity", "fold_2x17x16"),
          ("switch", "c3_two_sources"),
          ("out_row", "fold_3x9x7"), ("out_row", "fold_2x17x16")]


@pytest.mark.parametrize("broken,name", BREAKS)
def test_a_planted_break_changes_the_case_that_names_it(broken, name):
    """bounds / bounds_left: the ix < Wlim / ix >= 0 test dropped - the tap beyond the last (before the first) column reads the next row's first
    (the previous row's last) pixel, or the guard (the wide image's last tap column lies inside: only its ix = -1 is out of bounds);  parity: the
    class's shift 1 - py taken as py;  switch: the source switch one tile late - x0 is read behind its last channel;  out_row: without
    py * 2 Win - the odd rows are never written and the even ones twice."""
    c = G.CASES[name]
    got, ref = G.recipe(c, broken=broken).double(), G.problem(c)["t64"]
    differ = int(((got != ref) | torch.isnan(got)).sum())
    assert differ > 0
    if broken == "out_row":
        Win = G.geometry(c)["Win"]
        rows = torch.isnan(got).all(1).view(-1, 2 * Win)           # whole output rows of the image left NaN: every odd one
        assert bool(rows[1::2].all()) and not bool(rows[0::2].any())


def test_the_row_vector_index():
    """vec_index (igemm_tail.h:88): mode 1 is m / vG; mode 2 the header's ((m / vFS) * vS + m % vS) % vB, spelled out per (clip, frame,
    position) - and without the % vB the index leaves the vB rows of the vector (into the NaN guard) on the case that names it."""
    c = G.CASES["tail_whole_P1_vec2"]
    M = G.geometry(c)["M"]
    frames = G.VFS // G.VS
    want = [((clip * G.VS + s) % G.VB) for clip in range(M // G.VFS) for f in range(frames) for s in range(G.VS)]
    assert G.vec_rows(c, M).tolist() == want and G.problem(c)["vec"].shape[0] == G.VB
    assert int((G.vec_rows(c, M, broken="vec_mod") >= G.VB).sum()) == G.VFS
    c = G.CASES["tail_mixed_P1_vec1"]
    assert G.vec_rows(c, M).tolist() == [m // G.VG for m in range(M)] and G.problem(c)["vec"].shape[0] == -(-M // G.VG)


# ------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("entry", G.REFUSALS, ids=lambda e: e[0])
def test_refusals_come_from_the_plan(entry):
    G.refused(entry, lambda L, p: L.pt_igemm_plan(p, None, None, None))


def test_hooks_are_restored():
    from posetraj_amd import hip
    c = G.CASES["lin_whole"]
    auto = G.planned(c, -1, False)
    with pytest.raises(ZeroDivisionError):
        with G.hooks(2, 4, 0):
            assert G.planned(c, 2, False)[0] == 2
            1 / 0
    p = G.make_params(c, G.fake_bases(c))
    cfg, gm = ctypes.c_int32(), ctypes.c_int32()
    assert hip.lib().pt_igemm_plan(ctypes.byref(p), ctypes.byref(cfg), None, ctypes.byref(gm)) == 0
    assert (cfg.value, gm.value) == (auto[0], auto[2])
