"""The sampler extension (include/posetraj_sampler.h, ``pts_*``) and ``DPMPP2MDiscreteScheduler`` without a GPU: the two
prototypes, the host-side refusals, the identities of ``coefficients``, and the solver's order on a Gaussian toy problem in fp64.

The toy: data ``N(0, s^2)`` has the exact denoiser ``D(x, sigma) = x s^2 / (s^2 + sigma^2)`` and the probability-flow solution
``x(0) = x(sigma_0) s / sqrt(s^2 + sigma_0^2)``.  The recurrence ``x <- a x + b D_i + c D_{i-1}`` over the scheduler's own N-step sigma
table is compared with it; ``coefficients(i, first=True)`` on every step is the Euler sampler.  The two conditions asserted are
conditions on the formulas, not measurements of this code: second order beats first order by a clear factor from 15 steps on
(ratios 1.6 - 7.6 here), and halving the step size divides the error by about 4 (4.3 - 4.4 here).
"""
import inspect
import math

import pytest
import torch

from posetraj_amd import DPMPP2MDiscreteScheduler, EulerDiscreteScheduler, SVD_SCHEDULER_CONFIG, hip

STEP_COUNTS = (1, 2, 4, 25)


# ------------------------------------------------------------------------------------------------------- header and library
def test_sampler_entry_point_prototypes():
    """The two exact prototypes ``hip`` read from the header.  (The header's contract with the library: tests/test_abi_cpu.py.)"""
    protos = hip.ABIS["sampler"].prototypes
    assert protos["pts_cfg_multistep_step"] == ("int", ["const void*", "int32_t", "int32_t", "const float*"] + ["float"] * 5 + ["int32_t"] * 4 +
                                                ["float*", "float*", "void*"])
    assert protos["pts_multistep_step"] == ("int", ["const void*", "int32_t", "const float*"] + ["float"] * 5 + ["float*", "float*", "int64_t", "void*"])
    assert "sampler.hip" in hip.SOURCES


def test_sampler_entry_points_refuse_bad_arguments_on_the_host():
    """Null pointer, ``ldn = 3``, non-positive sizes and a non-finite scalar return non-zero before any launch, with the entry point's
    name in ``pt_last_error()`` (the pointers below are never dereferenced)."""
    L, C = hip.lib(), hip.checked()
    P, nan, inf = 256, float("nan"), float("inf")
    ok = dict(pred=P, f32=1, ldn=4, g=P, cs=0.5, co=-0.5, a=0.5, b=0.75, c=-0.25, Bc=1, F=2, h=3, w=5, lat=P, dp=P, st=None)
    cfg = lambda **kw: L.pts_cfg_multistep_step(*{**ok, **kw}.values())
    for bad, word in ((dict(pred=None), b"null pointer"), (dict(g=None), b"null pointer"), (dict(lat=None), b"null pointer"),
                      (dict(dp=None), b"null pointer"), (dict(ldn=3), b"ldn"), (dict(Bc=0), b"sizes"), (dict(F=-1), b"sizes"),
                      (dict(h=0), b"sizes"), (dict(w=0), b"sizes"), (dict(cs=nan), b"non-finite"), (dict(co=inf), b"non-finite"),
                      (dict(a=nan), b"non-finite"), (dict(b=-inf), b"non-finite"), (dict(c=nan), b"non-finite")):
        assert cfg(**bad) != 0, bad
        err = L.pt_last_error()
        assert b"pts_cfg_multistep_step" in err and word in err, (bad, err)
    okf = dict(mo=P, f32=0, x=P, cs=0.5, co=-0.5, a=0.5, b=0.75, c=0.0, dp=P, out=P, n=7, st=None)
    flat = lambda **kw: L.pts_multistep_step(*{**okf, **kw}.values())
    for bad, word in ((dict(mo=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(dp=None), b"null pointer"),
                      (dict(out=None), b"null pointer"), (dict(n=0), b"size"), (dict(n=-4), b"size"), (dict(cs=nan), b"non-finite"),
                      (dict(c=inf), b"non-finite")):
        assert flat(**bad) != 0, bad
        err = L.pt_last_error()
        assert b"pts_multistep_step" in err and word in err, (bad, err)
    with pytest.raises(RuntimeError, match="pts_cfg_multistep_step"):
        C.pts_cfg_multistep_step(*{**ok, "ldn": 3}.values())
    with pytest.raises(RuntimeError, match="pts_multistep_step"):
        C.pts_multistep_step(*{**okf, "a": nan}.values())


# ------------------------------------------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("N", STEP_COUNTS)
def test_coefficients_identities(N):
    s = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s.set_timesteps(N)
    sig = s._sigmas_host
    assert len(sig) == N + 1 and sig[-1] == 0.0
    c_skip, c_out, a, b, c = s.coefficients(0)
    ratio = sig[1] / sig[0]
    assert c == 0.0 and abs(a - ratio) <= 1e-15 and abs(b - (1.0 - ratio)) <= 1e-15            # the first step is the Euler step
    for i in range(N):
        c_skip, c_out, a, b, c = s.coefficients(i)
        assert all(isinstance(v, float) and math.isfinite(v) for v in (c_skip, c_out, a, b, c))
        assert abs(c_skip - 1.0 / (sig[i] ** 2 + 1.0)) <= 1e-15 and abs(c_out + sig[i] / math.sqrt(sig[i] ** 2 + 1.0)) <= 1e-15
        if sig[i + 1] > 0:
            assert abs(a + b + c - 1.0) <= 1e-12, (i, a, b, c)                                  # a constant denoiser's fixed point stays put
            assert abs(a - sig[i + 1] / sig[i]) <= 1e-15 and (c < 0.0 < b if i else c == 0.0)
            _, _, a1, b1, c1 = s.coefficients(i, first=True)                                    # any step without a history: Euler
            assert a1 == a and abs(b1 - (1.0 - a)) <= 1e-15 and c1 == 0.0
    assert s.coefficients(N - 1)[2:] == (0.0, 1.0, 0.0)                                         # the step to sigma' = 0 returns D
    with pytest.raises(IndexError):
        s.coefficients(N)
    with pytest.raises(IndexError):
        s.coefficients(-1)


def test_coefficients_follow_the_prediction_type():
    for ptype, want in (("v_prediction", lambda s: (1.0 / (s * s + 1.0), -s / math.sqrt(s * s + 1.0))), ("epsilon", lambda s: (1.0, -s)),
                        ("sample", lambda s: (0.0, 1.0))):
        s = DPMPP2MDiscreteScheduler(**{**SVD_SCHEDULER_CONFIG, "prediction_type": ptype})
        s.set_timesteps(4)
        for i in range(4):
            got, ref = s.coefficients(i)[:2], want(s._sigmas_host[i])
            assert abs(got[0] - ref[0]) <= 1e-15 and abs(got[1] - ref[1]) <= 1e-12 * max(1.0, abs(ref[1])), (ptype, i, got, ref)
    bad = DPMPP2MDiscreteScheduler(**{**SVD_SCHEDULER_CONFIG, "prediction_type": "flow"})
    bad.set_timesteps(4)
    with pytest.raises(ValueError, match="prediction_type"):
        bad.coefficients(0)


def test_later_steps_are_k_diffusions_dpmpp_2m():
    """``sample_dpmpp_2m`` written out: ``t = -ln sigma``, ``h = t' - t``, ``h_last = t - t_prev``, ``r = h_last / h``,
    ``x' = (sigma'/sigma) x - expm1(-h) ((1 + 1/(2r)) D - (1/(2r)) D_prev)`` - on numbers, against ``a x + b D + c D_prev``."""
    s = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s.set_timesteps(25)
    sig = s._sigmas_host
    x, D, Dp = 0.7, -1.3, 2.1
    for i in range(1, 24):
        t_prev, t, t_next = (-math.log(sig[j]) for j in (i - 1, i, i + 1))
        h, r = t_next - t, (t - t_prev) / (t_next - t)
        want = (sig[i + 1] / sig[i]) * x - math.expm1(-h) * ((1 + 1 / (2 * r)) * D - (1 / (2 * r)) * Dp)
        _, _, a, b, c = s.coefficients(i)
        assert abs(a * x + b * D + c * Dp - want) <= 1e-12, i


# ----------------------------------------------------------------------------------------------------------- the Gaussian toy
def _toy_error(N, s, second_order):
    sch = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    sch.set_timesteps(N)
    sig = sch._sigmas_host
    x, Dp = 1.0, 0.0
    for i in range(N):
        _, _, a, b, c = sch.coefficients(i) if second_order else sch.coefficients(i, first=True)
        D = x * s * s / (s * s + sig[i] ** 2)
        x, Dp = a * x + b * D + c * Dp, D
    return abs(x - s / math.sqrt(s * s + sig[0] ** 2))


@pytest.mark.parametrize("s", [0.5, 1.0, 3.0])
def test_gaussian_toy_second_order_beats_euler_and_converges_at_order_two(s):
    for N in (15, 20, 25, 50):
        assert _toy_error(N, s, True) <= _toy_error(N, s, False) / 1.3, (s, N, _toy_error(N, s, True), _toy_error(N, s, False))
    assert _toy_error(50, s, True) / _toy_error(100, s, True) >= 3.5


# ------------------------------------------------------------------------------------------------------------------ the class
def test_from_config_round_trips_and_the_class_inherits_the_tables():
    e = EulerDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s = DPMPP2MDiscreteScheduler.from_config(e.config)
    assert isinstance(s, EulerDiscreteScheduler) and s.order == 2 and e.order == 1
    assert dict(s.config) == dict(e.config) == dict(DPMPP2MDiscreteScheduler.from_config(s.config).config)
    assert dict(DPMPP2MDiscreteScheduler.from_config({**e.config, "unknown_key": 1}).config) == dict(e.config)
    for N in STEP_COUNTS:
        e.set_timesteps(N)
        s.set_timesteps(N)
        assert e._sigmas_host == s._sigmas_host and torch.equal(e.timesteps, s.timesteps) and float(e.init_noise_sigma) == float(s.init_noise_sigma)
    for name in ("set_timesteps", "scale_model_input", "add_noise", "init_noise_sigma", "__init__"):
        assert name not in vars(DPMPP2MDiscreteScheduler)                                       # inherited, not restated
    assert list(inspect.signature(DPMPP2MDiscreteScheduler.step).parameters) == ["self", "model_output", "timestep", "sample", "return_dict"]


def test_step_refuses_integer_timesteps_like_the_euler_class():
    x = torch.zeros(1, 2, 4, 3, 3)
    for cls in (EulerDiscreteScheduler, DPMPP2MDiscreteScheduler):
        s = cls(**SVD_SCHEDULER_CONFIG)
        s.set_timesteps(4)
        for t in (0, torch.tensor(0), torch.tensor(1, dtype=torch.int32)):
            with pytest.raises(ValueError, match="integer indices"):
                s.step(x, t, x)
    s = DPMPP2MDiscreteScheduler(**SVD_SCHEDULER_CONFIG)
    s.set_timesteps(4)
    with pytest.raises(RuntimeError, match="GPU"):                                              # no CPU path exists
        s.step(x, s.timesteps[0], x)
    with pytest.raises(TypeError):
        s.step(x, s.timesteps[0], x, s_churn=0.5)
