"""``autodiff.checkpoint`` on the host: the wrapper is tape logic only (no kernel of its own), so toy primitives over CPU tensors on
``AD.Tape`` / ``AD.Var`` pin it down - gradients equal to the plain tape's bit for bit, the segment function called exactly twice
(once when its output receives no gradient), the segment's intermediates dead right after the forward.  The toys accumulate with
a helper of their own: ``autodiff._acc``'s second add is a device kernel.  The toys exist twice - on ``Tape.record`` with the gradient
hand-over written out, and on ``Tape.op`` - and must agree bit for bit; ``Tape.op`` and ``Tape.backward(release=True)`` are pinned down
directly as well."""
import inspect
import weakref

import torch


def _acc(var, g):
    if var.need:
        var.g = g if var.g is None else var.g + g


def mul(AD, tape, a, b):
    out = AD.Var(a.v * b.v)

    def bwd():
        dy, out.g = out.g, None
        if dy is None:
            return
        _acc(a, dy * b.v)
        _acc(b, dy * a.v)

    tape.record(bwd)
    return out


def tanh(AD, tape, x, born=None):
    out = AD.Var(torch.tanh(x.v))
    if born is not None:
        born.append(weakref.ref(out.v))

    def bwd():
        dy, out.g = out.g, None
        if dy is not None:
            _acc(x, dy * (1 - out.v * out.v))

    tape.record(bwd)
    return out


def add(AD, tape, a, b):
    out = AD.Var(a.v + b.v)

    def bwd():
        dy, out.g = out.g, None
        if dy is not None:
            _acc(a, dy)
            _acc(b, dy)

    tape.record(bwd)
    return out


def mul_op(AD, tape, a, b):
    out = AD.Var(a.v * b.v)

    def bwd(dy):
        _acc(a, dy * b.v)
        _acc(b, dy * a.v)

    tape.op(out, bwd)
    return out


def tanh_op(AD, tape, x, born=None):
    out = AD.Var(torch.tanh(x.v))
    if born is not None:
        born.append(weakref.ref(out.v))
    tape.op(out, lambda dy: _acc(x, dy * (1 - out.v * out.v)))
    return out


def add_op(AD, tape, a, b):
    out = AD.Var(a.v + b.v)

    def bwd(dy):
        _acc(a, dy)
        _acc(b, dy)

    tape.op(out, bwd)
    return out


ON_RECORD, ON_OP = (mul, tanh, add), (mul_op, tanh_op, add_op)


def _leaves(AD, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [AD.Var(torch.randn(5, 7, generator=g, dtype=torch.float64)) for _ in range(3)]


def _network(AD, tape, x, w, c, wrap, calls, born=None, toys=ON_RECORD):
    """Two segments in a row; ``x`` is used inside the first segment and again after both, ``pre`` is produced on the outer tape
    before the segments and closed over by both, ``w`` is read by both segments."""
    mul, tanh, add = toys
    pre = tanh(AD, tape, c)

    def seg1(t):
        calls[0] += 1
        return mul(AD, t, tanh(AD, t, mul(AD, t, x, w), born), add(AD, t, pre, x))

    def seg2(t, h):
        calls[1] += 1
        return add(AD, t, tanh(AD, t, mul(AD, t, h, pre), born), mul(AD, t, h, w))

    h1 = wrap(tape, seg1)
    h2 = wrap(tape, lambda t: seg2(t, h1))
    return add(AD, tape, mul(AD, tape, h2, x), h1)


def _run(AD, wrap, born=None, toys=ON_RECORD, release=False):
    x, w, c = _leaves(AD)
    tape, calls = AD.Tape(), [0, 0]
    y = _network(AD, tape, x, w, c, wrap, calls, born, toys)
    forward_calls = list(calls)
    alive_after_forward = None if born is None else [r() is not None for r in born]
    y.g = torch.ones_like(y.v)
    if release:
        tape.backward(release=True)
    else:
        tape.backward()
    return y.v, (x.g, w.g, c.g), forward_calls, calls, alive_after_forward


def test_checkpoint_gradients_equal_the_plain_tape():
    from posetraj_amd import autodiff as AD
    y0, g0, _, calls0, _ = _run(AD, lambda tape, fn: fn(tape))
    y1, g1, fwd1, calls1, _ = _run(AD, AD.checkpoint)
    assert calls0 == [1, 1]
    assert fwd1 == [1, 1] and calls1 == [2, 2]                  # once in the forward, once in the reverse pass: exactly twice
    assert torch.equal(y0, y1)
    for a, b in zip(g0, g1):
        assert a is not None and torch.equal(a, b)
    # ... and they are the right gradients: torch autograd over the same expression
    x, w, c = (v.v.clone().requires_grad_(True) for v in _leaves(AD))
    pre = torch.tanh(c)
    h1 = torch.tanh(x * w) * (pre + x)
    h2 = torch.tanh(h1 * pre) + h1 * w
    (h2 * x + h1).sum().backward()
    for a, b in zip(g1, (x.grad, w.grad, c.grad)):
        assert torch.allclose(a, b, rtol=1e-12, atol=1e-12)


def test_checkpoint_frees_the_segment_after_the_forward():
    from posetraj_amd import autodiff as AD
    born = []
    _, _, _, _, alive = _run(AD, lambda tape, fn: fn(tape), born)
    assert alive == [True, True]                                # the plain tape keeps every intermediate until its reverse pass
    born = []
    _, _, _, calls, alive = _run(AD, AD.checkpoint, born)
    assert alive == [False, False]                              # dead right after the forward (recorded before backward started)
    assert len(born) == 4 and all(r() is None for r in born)    # the recomputed ones die with the local tape


def test_checkpoint_without_a_gradient_is_not_recomputed():
    from posetraj_amd import autodiff as AD
    x, w, _ = _leaves(AD, seed=1)
    tape, calls = AD.Tape(), [0]

    def seg(t):
        calls[0] += 1
        return tanh(AD, t, mul(AD, t, x, w))

    dead_end = AD.checkpoint(tape, seg)                         # nobody consumes it: its output receives no gradient
    y = mul(AD, tape, x, w)
    y.g = torch.ones_like(y.v)
    tape.backward()
    assert calls == [1] and dead_end.g is None
    assert torch.equal(x.g, w.v) and torch.equal(w.g, x.v)


def test_toys_on_tape_op_equal_the_toys_on_record():
    """The same network from primitives that leave the hand-over to ``Tape.op``: the gradients of ``x``, ``w`` and ``c`` and the
    segment call counts equal those of the hand-written protocol, on the plain tape and under ``AD.checkpoint``."""
    from posetraj_amd import autodiff as AD
    for wrap in (lambda tape, fn: fn(tape), AD.checkpoint):
        y0, g0, fwd0, calls0, _ = _run(AD, wrap, toys=ON_RECORD)
        y1, g1, fwd1, calls1, _ = _run(AD, wrap, toys=ON_OP)
        assert torch.equal(y0, y1) and fwd0 == fwd1 and calls0 == calls1
        for a, b in zip(g0, g1):
            assert a is not None and b is not None and torch.equal(a, b)


def test_tape_op_hands_the_gradient_over():
    from posetraj_amd import autodiff as AD
    tape, seen = AD.Tape(), []
    out, quiet = AD.Var(torch.zeros(3)), AD.Var(torch.zeros(3))
    tape.op(quiet, lambda dy: seen.append(("quiet", dy, quiet.g)))
    tape.op(out, lambda dy: seen.append(("out", dy, out.g)))
    g = torch.ones(3)
    out.g = g
    tape.backward()
    assert len(seen) == 1                                       # once for the output with a gradient, never for the one without
    name, dy, left = seen[0]
    assert name == "out" and dy is g and left is None           # already taken off the output when the closure runs
    assert out.g is None and quiet.g is None


def test_backward_release_keeps_the_order_and_drops_each_closure_as_it_has_run():
    from posetraj_amd import autodiff as AD

    def tape_of(log):
        """Three closures; the LAST recorded (first to run) is the only holder of a tensor, the one before it looks whether it is alive."""
        tape, held = AD.Tape(), torch.ones(4)
        ref = weakref.ref(held)
        tape.record(lambda: log.append(0))
        tape.record(lambda: log.append((1, ref() is not None)))
        tape.record(lambda: log.append((2, float(held.sum()))))
        return tape

    plain, released = [], []
    tape_of(plain).backward()
    tape = tape_of(released)
    tape.backward(release=True)
    assert plain == [(2, 4.0), (1, True), 0]                    # default: reversed order, closures (and what they hold) dropped at the end
    assert released == [(2, 4.0), (1, False), 0]                # the same order and results, the tensor dead before the next closure ran
    tape.backward()
    assert len(released) == 3                                   # nothing is left on the tape
    # ... and the same gradients on a whole network, plain and checkpointed
    for wrap in (lambda tape, fn: fn(tape), AD.checkpoint):
        _, g0, _, calls0, _ = _run(AD, wrap)
        _, g1, _, calls1, _ = _run(AD, wrap, release=True)
        assert calls0 == calls1 and all(torch.equal(a, b) for a, b in zip(g0, g1))


def test_trainer_takes_the_keyword():
    from posetraj_amd.training import ControlNetTrainer
    from posetraj_amd import train_graph as TG
    p = inspect.signature(ControlNetTrainer.__init__).parameters
    assert "gradient_checkpointing" in p and p["gradient_checkpointing"].default is False
    for cls in (TG.ControlNetGraph, TG.UNetDecoderGraph):
        q = inspect.signature(cls.run).parameters
        assert "checkpoint" in q and q["checkpoint"].default is False
