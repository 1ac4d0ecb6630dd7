"""``--use_8bit_adam`` on the device: ``pto_adamw8_f32`` / ``pto_adam8_dequant_f32`` against an fp64 restatement of one step of the
blockwise 8-bit AdamW (written here from the format's description, independent of the kernel), against ``pt_adamw_fused_f32`` where
both run the same fp32 statements (``torch.equal``), and ``ControlNetTrainer(use_8bit_adam=True)``: three steps, a forced skip, memory,
checkpoint resume.  bitsandbytes itself is not available: parity with the package is not claimed anywhere below.

Bounds (none is taken from what the kernel gives):
  parameters  |p - p64| <= 2e-6 (|p64| + lr/bc1 (|b1 deq1| + |(1 - b1) g'|) / denom64): about ten fp32 roundings of 6e-8 each,
              relative to the magnitudes of the terms, not to a cancelled sum;
  absmax      1e-6 relative to the block maximum of the fp64 |m| resp. v;
  codes       |book[code] - x| <= min_k |book[k] - x| + 4e-6 with x = m64 / absmax64' (fp32 quotient: a few 1e-7; ties are safe)."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HAND = [1, 320, 4095, 4096, 4232, 5000, 3 * 3 * 32 * 48]
SWEEP = 256 * 8 * 4 * 256                    # elements one wave-per-unit sweep of the grid covers: beyond it a wave walks several units
LONG = HAND + [SWEEP + 3 * 256 + 77]
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=3, inv_scale=1 / 256.0)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------- the restatement
def f32(x):
    return float(np.float32(x))


def restated_step(p, g, deq1, deq2, lr, b1, b2, eps, wd, step, inv_scale):
    """One AdamW step in fp64 over flat tensors, the moments given DEQUANTISED (``book[code] * absmax``, or the fp32 moments).  The
    hyper-parameters are the fp32 values the launch receives.  Returns ``p, m, v`` and the magnitude the parameter bound refers to (and that of m's two terms)."""
    lr, b1, b2, eps, wd, inv_scale = (f32(x) for x in (lr, b1, b2, eps, wd, inv_scale))
    bc1, bc2 = f32(1.0 - b1 ** step), 1.0 - b2 ** step
    p, g, deq1, deq2 = (t.double() for t in (p, g, deq1, deq2))
    gs = g * inv_scale
    m = b1 * deq1 + (1 - b1) * gs
    v = b2 * deq2 + (1 - b2) * gs * gs
    denom = v.sqrt() / f32(np.sqrt(bc2)) + eps
    pn = p * (1 - lr * wd) - (lr / bc1) * (m / denom)
    mmag = (b1 * deq1).abs() + ((1 - b1) * gs).abs()
    mag = pn.abs() + (lr / bc1) * mmag / denom
    return pn, m, v, mag, mmag


def block_max(x, segs):
    """Per 8-bit block (in block order) the maximum of ``x`` over the block's elements."""
    out = []
    for start, count, state, kind in segs:
        if kind:
            for o in range(0, count, 256):
                out.append(x[start + o:start + min(o + 256, count)].max())
    return torch.stack(out) if out else torch.zeros(0, dtype=x.dtype)


def expand(per_block, segs, n):
    """A per-block value as a flat tensor over the elements of the 8-bit parameters (0 elsewhere)."""
    out = torch.zeros(n, dtype=per_block.dtype)
    for start, count, state, kind in segs:
        if kind:
            for u, o in enumerate(range(0, count, 256)):
                out[start + o:start + min(o + 256, count)] = per_block[state + u]
    return out


def gather_codes(codes, segs, n):
    """The code buffer (256 per block) as a flat int64 tensor in the layout of p (0 elsewhere)."""
    out = torch.zeros(n, dtype=torch.int64)
    for start, count, state, kind in segs:
        if kind:
            out[start:start + count] = codes[256 * state:256 * state + count].long()
    return out


def check_codes(code_flat, x64, book, live8, what):
    """``|book[code] - x| <= min_k |book[k] - x| + 4e-6`` for every element of the 8-bit parameters."""
    b = book.double()
    x = x64[live8]
    got = (b[code_flat[live8]] - x).abs()
    idx = torch.searchsorted(b, x).clamp(1, 255)
    best = torch.minimum((b[idx] - x).abs(), (b[idx - 1] - x).abs())
    worst = float((got - best).max()) if x.numel() else 0.0
    print(f"{what}: worst excess distance to the nearest code {worst:.3e} over {x.numel()} elements")
    assert worst <= 4e-6, what


# ------------------------------------------------------------------------------------------------- a store built by hand
class Case:
    """A flat store over ``counts`` with a test-made state: random codes, absmax over 12 decades, some blocks with absmax 0; gradient
    magnitudes 1e-8 .. 1e2 across blocks, some blocks all zero (every third of those on a zero-absmax block); the padding between the
    parameters holds a sentinel in p."""
    SENTINEL = 123.0

    def __init__(self, counts, dev, seed=0, zero_state=False, sentinel=True):
        from posetraj_amd import hip
        from posetraj_amd.optim import create_dynamic_map, plan_8bit_state
        g = torch.Generator().manual_seed(seed)
        names = [f"p{i}" for i in range(len(counts))]
        shapes, offsets, n = {}, {}, 0
        for k, c in zip(names, counts):
            shapes[k], offsets[k] = (c,), n
            n += (c + 7) // 8 * 8
        self.n, self.plan = n, plan_8bit_state(names, shapes, offsets)
        self.segs = [s[1:5] for s in self.plan["segments"]]
        nb, nf, nw = self.plan["n_blocks"], self.plan["n_f32_alloc"], self.plan["n_work"]
        self.book1, self.book2 = create_dynamic_map(True), create_dynamic_map(False)
        self.live = torch.zeros(n, dtype=torch.bool)
        self.live8 = torch.zeros(n, dtype=torch.bool)
        for start, count, state, kind in self.segs:
            self.live[start:start + count] = True
            self.live8[start:start + count] = bool(kind)
        # per unit of 256 stored elements: gradient magnitude; per 8-bit block: absmax
        unit_of = torch.zeros(n, dtype=torch.int64)
        for (start, count, state, kind), seg in zip(self.segs, self.plan["segments"]):
            unit_of[start:start + count] = seg[5] + torch.arange(count) // 256
        gmag = torch.pow(10.0, torch.rand(nw, generator=g) * 10 - 8)
        gmag[::5] = 0.0
        self.p = torch.randn(n, generator=g)
        self.g = (torch.randn(n, generator=g) * gmag[unit_of]) * 256.0      # loss-scaled; inv_scale = 1 / 256 brings the magnitudes back
        self.g[~self.live] = 0.0
        self.p[~self.live] = self.SENTINEL if sentinel else 0.0
        self.am1 = torch.pow(10.0, torch.rand(nb, generator=g) * 12 - 10)
        self.am2 = torch.pow(10.0, torch.rand(nb, generator=g) * 12 - 10)
        dead = torch.zeros(nb, dtype=torch.bool)
        dead[::7] = True
        # the all-zero gradient units of the 8-bit parameters: every third of them also gets absmax 0 (a block that stays zero)
        zero_units = [state + u for (start, count, state, kind), seg in zip(self.segs, self.plan["segments"]) if kind
                      for u in range(-(-count // 256)) if gmag[seg[5] + u] == 0]
        dead[zero_units[::3]] = True
        self.am1[dead] = 0.0
        self.am2[dead] = 0.0
        self.c1 = torch.randint(0, 256, (nb * 256,), generator=g, dtype=torch.uint8)
        self.c2 = torch.randint(0, 256, (nb * 256,), generator=g, dtype=torch.uint8)
        self.m32 = torch.randn(nf, generator=g) * 0.1
        self.v32 = torch.rand(nf, generator=g) * 0.01
        if zero_state:
            self.c1.fill_(127); self.c2.fill_(0); self.am1.zero_(); self.am2.zero_(); self.m32.zero_(); self.v32.zero_()
        table = (hip.Adam8Segment * len(self.segs))(*[hip.Adam8Segment(*s[1:]) for s in self.plan["segments"]])
        self.table = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        self.dev = dev
        self.d = {k: getattr(self, k).to(dev) for k in ("p", "g", "c1", "c2", "am1", "am2", "book1", "book2", "m32", "v32")}
        self.d["mirror"] = torch.zeros(n, dtype=torch.float16, device=dev)

    def deq(self):
        """The state as flat fp32 moments, computed here: one fp32 product per element, the fp32 moments copied."""
        m = self.book1[gather_codes(self.c1, self.segs, self.n)] * expand(self.am1, self.segs, self.n)
        v = self.book2[gather_codes(self.c2, self.segs, self.n)] * expand(self.am2, self.segs, self.n)
        m[~self.live8], v[~self.live8] = 0.0, 0.0
        for start, count, state, kind in self.segs:
            if not kind:
                m[start:start + count], v[start:start + count] = self.m32[state:state + count], self.v32[state:state + count]
        return m, v

    def seg_ptr(self, table=None):
        from posetraj_amd import hip
        return ctypes.cast((self.table if table is None else table).data_ptr(), ctypes.POINTER(hip.Adam8Segment))

    def state_args(self, d=None):
        d = d or self.d
        ptr = lambda t: t.data_ptr() if t.numel() else None
        return (ptr(d["c1"]), ptr(d["c2"]), ptr(d["am1"]), ptr(d["am2"]), d["book1"].data_ptr(), d["book2"].data_ptr(), ptr(d["m32"]), ptr(d["v32"]),
                self.seg_ptr(), len(self.segs), self.plan["n_work"])

    def extents(self):
        return (self.n, self.plan["n_blocks"], self.plan["n_f32_alloc"])

    def step(self, d=None, shadow=None, omd=0.0, mirror=True, zero_grad=1, hyper=HYPER):
        from posetraj_amd import hip, ops
        d = d or self.d
        h = hyper
        return hip.lib().pto_adamw8_f32(d["p"].data_ptr(), d["g"].data_ptr(), *self.state_args(d), *self.extents(), h["lr"], h["b1"], h["b2"], h["eps"],
                                       h["wd"], h["step"], h["inv_scale"], d["mirror"].data_ptr() if mirror else None, zero_grad,
                                       None if shadow is None else shadow.data_ptr(), omd, ops._stream())

    def dequant(self, d=None, fill=0.0):
        from posetraj_amd import hip, ops
        d = d or self.d
        m, v = torch.full((self.n,), fill, device=self.dev), torch.full((self.n,), fill, device=self.dev)
        a = self.state_args(d)
        hip.check(hip.lib().pto_adam8_dequant_f32(*a, *self.extents(), m.data_ptr(), v.data_ptr(), ops._stream()), "pto_adam8_dequant_f32")
        return m.cpu(), v.cpu()


def fused_args(hyper=HYPER):
    h = hyper
    return (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], h["inv_scale"])


@pytest.fixture(scope="module")
def long_case(dev):
    """The long list, stepped once; the fp64 restatement of that step is computed once and shared."""
    from posetraj_amd import hip
    c = Case(LONG, dev, seed=1)
    deq1, deq2 = c.deq()
    got_deq = c.dequant(fill=-7.0)
    hip.check(c.step(), "pto_adamw8_f32")
    out = {k: v.cpu() for k, v in c.d.items()}
    ref = restated_step(c.p, c.g, deq1, deq2, **HYPER)
    return dict(c=c, deq=(deq1, deq2), got_deq=got_deq, out=out, ref=ref)


# ------------------------------------------------------------------------------------------------- the kernel
def test_one_step_against_the_fp64_restatement(long_case):
    c, out = long_case["c"], long_case["out"]
    p64, m64, v64, mag, mmag = long_case["ref"]
    live, live8, segs, n = c.live, c.live8, c.segs, c.n
    for k in ("p", "am1", "am2", "m32", "v32"):
        assert torch.isfinite(out[k]).all(), k
    # parameters
    err = (out["p"].double() - p64).abs()[live]
    ratio = float((err / mag[live].clamp_min(1e-300)).max())
    print(f"parameters: worst |p - p64| / magnitude {ratio:.3e} over {int(live.sum())} elements (bound 2e-6)")
    assert ratio <= 2e-6
    assert torch.equal(out["p"][~live], c.p[~live]) and bool((c.p[~live] == Case.SENTINEL).all()) and int((~live).sum()) > 0      # padding untouched
    assert float(out["g"].abs().max()) == 0.0                                                                                    # zeroed
    assert torch.equal(out["mirror"][live], out["p"][live].half())
    # absmax
    want1, want2 = block_max(m64.abs(), segs), block_max(v64, segs)
    for name, got, want in (("absmax1", out["am1"].double(), want1), ("absmax2", out["am2"].double(), want2)):
        rel = float(((got - want).abs() / want.clamp_min(1e-300)).max())
        print(f"{name}: worst relative distance to the fp64 block maximum {rel:.3e} over {want.numel()} blocks (bound 1e-6)")
        assert rel <= 1e-6 and torch.equal(got == 0, want == 0), name
    zero_blocks = want1 == 0
    assert int(zero_blocks.sum()) > 0 and torch.equal(zero_blocks, want2 == 0)
    # codes
    code1, code2 = gather_codes(out["c1"], segs, n), gather_codes(out["c2"], segs, n)
    a1, a2 = expand(want1, segs, n), expand(want2, segs, n)
    x1 = torch.where(a1 > 0, m64 / a1.clamp_min(1e-300), torch.zeros_like(m64))
    x2 = torch.where(a2 > 0, v64 / a2.clamp_min(1e-300), torch.zeros_like(v64))
    check_codes(code1, x1, c.book1, live8, "exp_avg codes")
    check_codes(code2, x2, c.book2, live8, "exp_avg_sq codes")
    zero_el = live8 & (a1 == 0)
    assert int(zero_el.sum()) > 0 and bool((code1[zero_el] == 127).all()) and bool((code2[zero_el] == 0).all())                   # the code of 0.0
    # the small parameters' fp32 moments: the restatement's m and v, rounded once
    for start, count, state, kind in segs:
        if not kind:
            for got, want, scale in ((out["m32"], m64, mmag), (out["v32"], v64, v64)):         # (m may cancel: relative to its terms)
                e = (got[state:state + count].double() - want[start:start + count]).abs()
                assert float((e / scale[start:start + count].clamp_min(1e-300)).max()) <= 1e-6
    # what the next step would read is finite
    assert torch.isfinite(c.book1[code1] * expand(out["am1"], segs, n)).all() and torch.isfinite(c.book2[code2] * expand(out["am2"], segs, n)).all()


def test_dequant_is_book_times_absmax(long_case):
    c = long_case["c"]
    (m, v), (gm, gv) = long_case["deq"], long_case["got_deq"]
    assert torch.equal(gm[c.live], m[c.live]) and torch.equal(gv[c.live], v[c.live])
    assert bool((gm[~c.live] == -7.0).all()) and bool((gv[~c.live] == -7.0).all())                   # the padding is not written


@pytest.mark.parametrize("counts", [HAND, LONG], ids=["hand", "long"])
def test_first_step_from_the_zero_state_equals_the_fp32_pass(dev, counts):
    """m = v = 0 on both sides, the same statements: parameters, fp16 mirror, zeroed gradient and the EMA shadow are bit-identical
    to ``pt_adamw_fused_f32`` / ``pt_adamw_ema_f32`` on copies of the same buffers."""
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    c = Case(counts, dev, seed=2, zero_state=True, sentinel=False)
    n = c.n
    hyper = dict(HYPER, step=1)
    s0 = (c.p * 1.001).to(dev)
    omd = 9 / 11
    for with_ema in (False, True):
        a = {k: v.clone() for k, v in c.d.items()}
        sa = s0.clone()
        hip.check(c.step(a, shadow=sa if with_ema else None, omd=omd, hyper=hyper), "pto_adamw8_f32")
        b = [c.d["p"].clone(), c.d["g"].clone(), torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
        hb, sb = torch.zeros(n, dtype=torch.float16, device=dev), s0.clone()
        if with_ema:
            hip.check(L.pt_adamw_ema_f32(*(t.data_ptr() for t in b), n, *fused_args(hyper), hb.data_ptr(), 1, sb.data_ptr(), omd, st), "pt_adamw_ema_f32")
        else:
            hip.check(L.pt_adamw_fused_f32(*(t.data_ptr() for t in b), n, *fused_args(hyper), hb.data_ptr(), 1, st), "pt_adamw_fused_f32")
        assert torch.equal(a["p"], b[0]) and not torch.equal(a["p"], c.d["p"])
        assert torch.equal(a["mirror"], hb) and float(a["g"].abs().max()) == 0.0 == float(b[1].abs().max())
        assert torch.equal(sa, sb) and (with_ema == (not torch.equal(sa, s0)))
        # the new state decodes to the fp32 pass's moments within half the widest gap of the book (times the block's absmax)
        m, v = c.dequant(a)
        live8 = c.live8 & (expand(a["am1"].cpu(), c.segs, n) > 0)
        am = expand(a["am1"].cpu(), c.segs, n)
        half_gap = float((c.book1[1:] - c.book1[:-1]).max()) / 2 + 1e-6
        assert int(live8.sum()) > 0 and float(((m - b[2].cpu()).abs()[live8] / am[live8]).max()) <= half_gap


def test_small_parameters_over_three_steps_equal_the_fp32_pass_on_their_spans(dev):
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    c = Case(HAND, dev, seed=3)
    small = [(start, count, state) for start, count, state, kind in c.segs if not kind]
    assert [s[1] for s in small] == [1, 320, 4095]
    ref = []
    for start, count, state in small:
        n4 = (count + 3) // 4 * 4
        ref.append([c.d["p"][start:start + n4].clone(), None, c.d["m32"][state:state + n4].clone(), c.d["v32"][state:state + n4].clone()])
    gen = torch.Generator().manual_seed(4)
    for k in range(3):
        hyper = dict(HYPER, step=k + 1)
        grad = torch.randn(c.n, generator=gen) * 25.0
        grad[~c.live] = 0.0
        c.d["g"].copy_(grad)
        for (start, count, state), r in zip(small, ref):
            n4 = (count + 3) // 4 * 4
            r[1] = c.d["g"][start:start + n4].clone()
            hip.check(L.pt_adamw_fused_f32(*(t.data_ptr() for t in r), n4, *fused_args(hyper), None, 0, st), "pt_adamw_fused_f32")
        hip.check(c.step(hyper=hyper), "pto_adamw8_f32")
        for (start, count, state), r in zip(small, ref):
            assert torch.equal(c.d["p"][start:start + count], r[0][:count]), (k, count)
            assert torch.equal(c.d["m32"][state:state + count], r[2][:count]) and torch.equal(c.d["v32"][state:state + count], r[3][:count]), (k, count)
    assert bool((c.d["p"].cpu()[~c.live] == Case.SENTINEL).all())


def test_argument_errors(dev):
    from posetraj_amd import hip, ops
    L, st = hip.lib(), ops._stream()
    c = Case(HAND, dev, seed=5)
    d, h = c.d, HYPER
    tail = (h["lr"], h["b1"], h["b2"], h["eps"], h["wd"], h["step"], h["inv_scale"], None, 1, None, 0.0, st)
    a = list(c.state_args())
    before = d["p"].clone()
    no_book = a[:4] + [None] + a[5:]
    assert L.pto_adamw8_f32(d["p"].data_ptr(), d["g"].data_ptr(), *no_book, *c.extents(), *tail) != 0 and b"qmap" in L.pt_last_error()
    assert L.pto_adamw8_f32(d["p"].data_ptr() + 4, d["g"].data_ptr(), *a, *c.extents(), *tail) != 0 and b"aligned" in L.pt_last_error()
    assert L.pto_adamw8_f32(d["p"].data_ptr(), d["g"].data_ptr(), *a, c.n - 2, *c.extents()[1:], *tail) != 0 and b"multiple of 4" in L.pt_last_error()
    no_state = [None] + a[1:]
    assert L.pto_adamw8_f32(d["p"].data_ptr(), d["g"].data_ptr(), *no_state, *c.extents(), *tail) != 0 and b"state1" in L.pt_last_error()
    m = torch.zeros(c.n, device=dev)
    assert L.pto_adam8_dequant_f32(*a[:5], None, *a[6:], *c.extents(), m.data_ptr(), m.data_ptr(), st) != 0 and b"qmap" in L.pt_last_error()
    assert L.pto_adam8_dequant_f32(*a, *c.extents(), m.data_ptr() + 2, m.data_ptr(), st) != 0 and b"aligned" in L.pt_last_error()
    assert torch.equal(d["p"], before)                        # a refused call launches nothing


# ------------------------------------------------------------------------------------------------- the trainer
def _flat_from_named(P, named):
    """name -> tensor in torch's shape, as a flat CPU buffer in the store's layout (0 between the parameters)."""
    flat = torch.zeros(P.numel, dtype=torch.float32)
    for k in P.names:
        P.shaped(P.raw(flat, k), k).copy_(named[k].cpu())
    return flat


@pytest.fixture(scope="module")
def run(dev, golden, tmp_path_factory):
    """Three optimizer steps of an 8-bit trainer on the tiny networks and the ``train_grads`` inputs.  ``loss_and_grads`` and
    ``optimizer_step`` are called separately: the gradients and the previous state (through the dequant entry and the raw buffers)
    are read in between.  A plain fp32 trainer takes the same three steps; at step 1 it is handed the 8-bit trainer's gradient
    buffer, so that the comparison of the first update does not depend on the reverse pass summing in the same order twice."""
    from posetraj_amd.training import ControlNetTrainer
    from tests.test_backward_gpu import _nets
    g = golden("train_grads")
    cn_o, un_o, un, cfg = _nets(dev)
    t = lambda n: torch.from_numpy(g[n])
    draws = dict(noise=t("noise"), sigmas=t("sigmas"), random_p=t("random_p"), ran_idx=int(g["ran_idx"]))
    batch = (t("latents"), t("emb"), torch.tensor([127.0]), t("traj"))
    sd0 = {k: v.clone() for k, v in cn_o.state_dict().items()}
    kw = dict(learning_rate=2e-4, conditioning_dropout_prob=0.1, loss_scale=4096.0)
    tr = ControlNetTrainer(cfg, sd0, un, **kw, use_8bit_adam=True)
    fp = ControlNetTrainer(cfg, sd0, un, **kw)
    P, A = tr.params, tr.optimizer
    ck = str(tmp_path_factory.mktemp("adam8") / "checkpoint-2")
    ck32 = str(tmp_path_factory.mktemp("adam8") / "checkpoint-1")
    steps = []
    for i in range(3):
        tr.loss_and_grads(*batch, **draws)
        rec = dict(p=P.flat.cpu(), grads=_flat_from_named(P, tr.gradients()), raw_grad=P.grad.clone(), deq=tuple(x.cpu() for x in A.dequantize()),
                   inv_scale=1.0 / (tr._accum_scale * tr.world))
        assert tr.optimizer_step() is True
        rec["p_new"] = P.flat.cpu()
        rec["state"] = {k: v.clone() for k, v in A.state_dict().items()}
        steps.append(rec)
        fp.loss_and_grads(*batch, **draws)
        if i == 0:
            fp.params.grad.copy_(rec["raw_grad"])
        assert fp.optimizer_step() is True
        if i == 0:
            p32_first = fp.params.flat.cpu()
            fp.save_state(ck32)
        if i == 1:
            tr.save_state(ck)
    return dict(tr=tr, fp=fp, steps=steps, p32_first=p32_first, ck=ck, ck32=ck32, nets=(un, cfg, sd0, kw), batch=batch, draws=draws)


DRIFT_RECORDED = 1.308e-4    # relative L2 distance from the fp32 trainer after three steps on one MI355X (profiles/r08/train_step_adam8bit_ab.txt)


def test_three_trainer_steps_follow_the_restatement(run):
    tr = run["tr"]
    P, A = tr.params, tr.optimizer
    assert A.kind == "adamw8bit" and A.exp_avg.numel() == A.exp_avg_sq.numel() == A.plan["n_f32_alloc"] < P.numel      # no full-size moment buffer
    assert not any(hasattr(P, name) for name in ("exp_avg", "exp_avg_sq", "adam8")) and (tr.optimizer_steps, tr.skipped_steps) == (3, 0)
    live = torch.zeros(P.numel, dtype=torch.bool)
    for k, (o, n) in P.spans().items():
        live[o:o + n] = True
    assert A.plan["n_blocks"] > 0 and A.plan["n_f32"] > 0                                            # both kinds of state are in play
    for i, rec in enumerate(run["steps"]):
        hyper = dict(lr=2e-4, b1=0.9, b2=0.999, eps=1e-8, wd=1e-2, step=i + 1, inv_scale=1.0)       # gradients() are already un-scaled
        p64, m64, v64, mag, _ = restated_step(rec["p"], rec["grads"], rec["deq"][0], rec["deq"][1], **hyper)
        ratio = float(((rec["p_new"].double() - p64).abs()[live] / mag[live].clamp_min(1e-300)).max())      # (a parameter at 0 with gradient 0: 0 / 1e-300)
        print(f"trainer step {i + 1}: worst |p - p64| / magnitude {ratio:.3e} (bound 2e-6)")
        # gradients() multiplies by 1 / scale where the kernel multiplies the raw gradient by inv_scale: the same power of two
        assert rec["inv_scale"] == 1 / 4096.0 and ratio <= 2e-6, i
        assert not torch.equal(rec["p_new"], rec["p"])
    first = run["steps"][0]
    assert float(first["deq"][0].abs().max()) == 0.0 == float(first["deq"][1].abs().max())           # a fresh trainer: the zero state
    assert torch.equal(first["p_new"], run["p32_first"])                                             # step 1 == the plain fp32 trainer's
    a, b = tr.params.flat.double().cpu()[live], run["fp"].params.flat.double().cpu()[live]
    drift = float((a - b).norm() / b.norm())
    print(f"drift after three steps: relative L2 distance to the fp32 trainer {drift:.3e}")
    if DRIFT_RECORDED is not None:
        assert drift <= 10 * DRIFT_RECORDED                                                          # a guard, not a parity claim


def test_a_forced_skip_leaves_parameters_and_state_alone(run, dev):
    from posetraj_amd.training import ControlNetTrainer
    un, cfg, sd0, kw = run["nets"]
    tr = ControlNetTrainer(cfg, sd0, un, **kw, use_8bit_adam=True, use_ema=True)
    assert tr.step(*run["batch"], **run["draws"])["stepped"] is True                                 # a state that is not all zeros
    A = tr.optimizer
    p0, s0, st0 = tr.params.flat.clone(), tr.ema.shadow.clone(), {k: v.clone() for k, v in A.state_dict().items()}
    tr.loss_and_grads(*run["batch"], **run["draws"])
    assert tr.optimizer_step(grad_norm=float("inf")) is False
    assert torch.equal(tr.params.flat, p0) and float(tr.params.grad.abs().max()) == 0.0
    st1 = A.state_dict()
    assert set(st0) == set(st1) and all(torch.equal(st0[k], st1[k]) for k in st0)
    assert tr.loss_scale == 2048.0 and (tr.optimizer_steps, tr.skipped_steps) == (1, 1)
    assert tr.ema.optimization_step == 2 and not torch.equal(tr.ema.shadow, s0)                      # the shadow still moves (decay 2/11)


def test_fused_and_separate_ema_give_the_same_numbers(run, dev):
    """``ema_fused`` is honoured by the 8-bit pass: the EMA inside ``pto_adamw8_f32`` or as ``pt_ema_update_f32`` behind it (both
    trainers step on the same gradient buffer)."""
    from posetraj_amd.training import ControlNetTrainer
    un, cfg, sd0, kw = run["nets"]
    x = ControlNetTrainer(cfg, sd0, un, **kw, use_8bit_adam=True, use_ema=True)
    y = ControlNetTrainer(cfg, sd0, un, **kw, use_8bit_adam=True, use_ema=True)
    y.ema_fused = False
    for i in range(2):                                        # EMA decay 0, then 2/11
        for t in (x, y):
            t.loss_and_grads(*run["batch"], **run["draws"])
        y.params.grad.copy_(x.params.grad)
        assert x.optimizer_step() is True and y.optimizer_step() is True
        assert torch.equal(x.params.flat, y.params.flat) and torch.equal(x.ema.shadow, y.ema.shadow), i
        assert not torch.equal(x.ema.shadow, x.params.flat) or i == 0
    sx, sy = x.optimizer.state_dict(), y.optimizer.state_dict()
    assert all(torch.equal(sx[k], sy[k]) for k in sx)


def test_memory_the_full_size_moments_are_gone(run, dev):
    from posetraj_amd.training import ControlNetTrainer
    un, cfg, sd0, kw = run["nets"]
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    a = ControlNetTrainer(cfg, sd0, un, **kw)
    grown32 = torch.cuda.memory_allocated() - before
    before = torch.cuda.memory_allocated()
    b = ControlNetTrainer(cfg, sd0, un, **kw, use_8bit_adam=True)
    grown8 = torch.cuda.memory_allocated() - before
    n, state_bytes = b.params.numel, b.optimizer.plan["state_bytes"]
    print(f"memory: fp32 trainer {grown32} B, 8-bit trainer {grown8} B, difference {grown32 - grown8} B, planner says {8 * n - state_bytes} B")
    assert abs((grown32 - grown8) - (8 * n - state_bytes)) < (1 << 21)
    assert b.optimizer.kind == "adamw8bit" and b.optimizer.exp_avg.numel() == b.optimizer.plan["n_f32_alloc"] < n
    assert not any(hasattr(t.params, name) for t in (a, b) for name in ("exp_avg", "exp_avg_sq", "adam8"))
    assert a.optimizer.exp_avg.numel() == n and a.optimizer.kind == "adamw"
    assert 8 * n - state_bytes > 0.7 * 8 * n


def test_resume_continues_bit_for_bit_and_the_kinds_do_not_mix(run, dev):
    from posetraj_amd.training import ControlNetTrainer
    un, cfg, sd0, kw = run["nets"]
    ck, ck32 = run["ck"], run["ck32"]
    assert sorted(os.listdir(ck)) == ["controlnet", "optimizer.safetensors", "trainer_state.json"]
    assert sorted(os.listdir(ck32)) == ["controlnet", "optimizer.safetensors", "trainer_state.json"]   # an fp32 checkpoint is what it was
    s8, s32 = json.load(open(os.path.join(ck, "trainer_state.json"))), json.load(open(os.path.join(ck32, "trainer_state.json")))
    assert s8["optimizer"] == "adamw8bit" and s8["optimizer_block_size"] == 256 and "optimizer" not in s32
    b = ControlNetTrainer(cfg, sd0, un, **kw, use_8bit_adam=True)
    b.load_state(ck)
    third = run["steps"][2]
    assert b.optimizer_steps == 2 and torch.equal(b.params.flat.cpu(), third["p"])
    deq = b.optimizer.dequantize()
    assert torch.equal(deq[0].cpu(), third["deq"][0]) and torch.equal(deq[1].cpu(), third["deq"][1])
    b.loss_and_grads(*run["batch"], **run["draws"])
    same = torch.equal(b.params.grad, third["raw_grad"])
    print(f"resume: the reverse pass reproduced the uninterrupted run's gradient buffer bit for bit: {same}")
    b.params.grad.copy_(third["raw_grad"])                    # the step under test is the optimizer's: both runs take it on the same gradients
    assert b.optimizer_step() is True
    assert torch.equal(b.params.flat.cpu(), third["p_new"])
    got = b.optimizer.state_dict()
    assert set(got) == set(third["state"]) and all(torch.equal(got[k], third["state"][k]) for k in got)
    with pytest.raises(ValueError, match="'adamw8bit'.*'adamw'"):
        ControlNetTrainer(cfg, sd0, un, **kw).load_state(ck)
    with pytest.raises(ValueError, match="'adamw'.*'adamw8bit'"):
        b.load_state(ck32)
