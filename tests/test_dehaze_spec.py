"""The dehazing's specification (tests/dehaze_spec.py) against itself and against a plain float64 restatement of the same
definition: the identities hold byte for byte, the fixed point costs what DESIGN.md "Dehazing" says it costs, and on every
synthetic hazy scene the dehazed picture is closer to the haze-free one than the hazy picture is."""
import numpy as np
import pytest

import dehaze_cases as C
import dehaze_spec as S

# measured on the four committed scenes (printed by test_fixed_point_against_float64; DESIGN.md "Dehazing" quotes them):
# the largest |J - J_float| is 1 grey level, the largest |t - t_float| 2.327e-4 (the 12 fractional bits of p and of t, and
# the 12 of a_q under the guide's 255).  The bounds: one grey level more; twice the measured value.
MEASURED_J, MEASURED_T = 1, 2.327e-4
BOUND_J, BOUND_T = MEASURED_J + 1, 2 * MEASURED_T


def float_box(a, r):
    """The window's sum, border replicated, by plain summation."""
    p = np.pad(a, r, mode="edge")
    h, w = a.shape
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1))


def float_dehaze(img, radius, omega_q, t0_q, refine, eps):
    """The same definition in float64: same windows, same A, the guided filter in means, floor(x + 0.5) at the end."""
    I = S.planes(img).astype(np.float64)
    A = S.atmospheric_light(img, radius).astype(np.float64)
    n = np.minimum(1.0, (I / A).min(axis=2))
    p = 1.0 - (omega_q / 256.0) * S.window_min(n, radius)
    t = p
    if refine:
        G = S.grey(img).astype(np.float64)
        W = float((2 * refine + 1) ** 2)
        mG, mp = float_box(G, refine) / W, float_box(p, refine) / W
        cov = float_box(G * p, refine) / W - mG * mp
        var = float_box(G * G, refine) / W - mG * mG
        a = cov / (var + eps)
        b = mp - a * mG
        t = float_box(a, refine) / W * G + float_box(b, refine) / W
    t = np.clip(t, t0_q / float(S.ONE), 1.0)
    J = np.clip(np.floor(A + (I - A) / t[..., None] + 0.5), 0, 255).astype(np.uint8)
    return J.reshape(np.asarray(img).shape), t


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_identities(name):
    img, p = C.cases()[name]
    J, _, _ = S.dehaze_q(img, **dict(p, omega_q=0))
    assert J.tobytes() == img.tobytes()                                    # no haze taken out: t = 1
    J, t, _ = S.dehaze_q(img, **dict(p, t0_q=S.ONE))
    assert J.tobytes() == img.tobytes() and (t == S.ONE).all()             # the floor at 1
    q = dict(p, refine=0)
    A = S.atmospheric_light(img, q["radius"])
    raw = S.raw_transmission(img, A, q["radius"], q["omega_q"])
    assert S.transmission_q(img, **q).tobytes() == np.clip(raw, q["t0_q"], S.ONE).astype(np.uint16).tobytes()


def test_fixed_point_against_float64():
    worst_j = worst_t = 0.0
    for name in C.SCENES:
        _, I, _, p = C.scene(name)
        J, t, _ = S.dehaze_q(I, **p)
        Jf, tf = float_dehaze(I, **p)
        dj = int(np.abs(J.astype(int) - Jf.astype(int)).max())
        dt = float(np.abs(t / float(S.ONE) - tf).max())
        print(f"{name}: radius {p['radius']} refine {p['refine']}: max |J - J_float| = {dj}, max |t - t_float| = {dt:.3e}")
        worst_j, worst_t = max(worst_j, dj), max(worst_t, dt)
    print(f"worst: J {worst_j:.0f}, t {worst_t:.3e}")
    assert worst_j <= BOUND_J and worst_t <= BOUND_T


@pytest.mark.parametrize("name", sorted(C.SCENES))
def test_the_dehazed_picture_is_closer_to_the_haze_free_one(name):
    J_true, I, t_true, p = C.scene(name)
    J, t, A = S.dehaze_q(I, **p)
    mae = lambda a: float(np.abs(a.astype(np.float64) - J_true).mean())      # noqa: E731
    print(f"{name}: mean absolute error {mae(I):.1f} hazy -> {mae(J):.1f} dehazed; A {A.tolist()} (true {C.SCENE_A.astype(int).tolist()})")
    assert mae(J) < mae(I)


def test_argument_rules():
    assert S.arguments() == (7, 243, 410, 30, 64)
    assert S.arguments(t0=0.0)[2] == 1 and S.arguments(omega=1.0)[1] == 256 and S.arguments(omega=0.0)[1] == 0 and S.arguments(t0=1.0)[2] == S.ONE
    for bad in (dict(radius=-1), dict(radius=33), dict(refine=33), dict(refine=-1), dict(eps=0), dict(eps=65536), dict(omega=1.01),
                dict(omega=-0.1), dict(t0=1.5), dict(t0=float("nan"))):
        with pytest.raises(ValueError):
            S.arguments(**bad)
