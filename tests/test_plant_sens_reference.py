"""The yardstick of the plant-step sensitivities (tests/plant_sens_reference.py) against the CPU oracle: its value path is the
oracle's plant step, its x and u columns are central differences of that step, its theta columns central differences between
oracles built with theta_j (1 +- 1e-4).  No GPU; passes with or without the device kernels."""
import numpy as np
import pytest

import param_sens_reference as PR
import plant_sens_reference as PSR


@pytest.fixture(scope="module")
def states(pkg, tables):
    x = pkg.sample_x0(tables, 24, seed=23)
    u = np.random.default_rng(5).uniform(-1.0, 1.0, size=(24, 2)) * np.array([0.5, 1.0])
    return x, u


@pytest.fixture(scope="module")
def ref(states, tables):
    """The reference at n_sub = 4 (24 states) and 400 (6 states), computed once."""
    x, u = states
    return {4: PSR.plant_sensitivities(x, u, tables, n_sub=4), 400: PSR.plant_sensitivities(x[:6], u[:6], tables, n_sub=400)}


@pytest.mark.parametrize("n_sub,M", [(4, 24), (400, 6)])
def test_value_path_is_the_oracles_plant_step(states, ref, oracle, n_sub, M):
    x, u = states
    want = oracle.plant_step(x[:M], u[:M], n_sub=n_sub)
    err = np.abs(ref[n_sub]["x_next"] - want).max()
    print(f"n_sub={n_sub}: max|x_next - oracle| = {err:.3e}")
    assert err <= 1e-12


@pytest.mark.parametrize("n_sub,M", [(4, 24), (400, 6)])
def test_state_and_input_columns_against_central_differences(states, ref, oracle, n_sub, M):
    x, u = states
    x, u = x[:M], u[:M]
    S = np.concatenate([ref[n_sub]["dx"], ref[n_sub]["du"]], axis=2)  # (M, 8, 10)
    xu = np.concatenate([x, u], axis=1)
    fd = np.zeros_like(S)
    for j in range(10):
        h = 1e-5 * np.maximum(1.0, np.abs(xu[:, j]))
        p, m = xu.copy(), xu.copy()
        p[:, j] += h
        m[:, j] -= h
        fd[:, :, j] = (oracle.plant_step(p[:, :8], p[:, 8:], n_sub=n_sub) - oracle.plant_step(m[:, :8], m[:, 8:], n_sub=n_sub)) / (2 * h)[:, None]
    err = np.abs(S - fd).max(axis=(1, 2)) / np.abs(S).max(axis=(1, 2))
    print(f"n_sub={n_sub}: max error of the x, u columns / max|S| = {err.max():.3e}")
    assert err.max() <= 1e-5


def test_theta_columns_against_perturbed_oracles(states, ref, orc, tables):
    """Per instance over the 8 x 16 block, every column in units of its parameter (S_j theta_j, the derivative w.r.t. log theta_j
    that a relative step measures): the columns' natural scales differ by ten orders of magnitude."""
    x, u = states
    th0 = PR.theta_values(orc.default_params())
    assert np.array_equal(th0, PR.theta_values())
    S = ref[4]["dtheta"] * th0
    fd = np.zeros_like(S)
    for j in range(PR.NT):
        out = []
        for sgn in (1.0, -1.0):
            p = PR.set_theta(orc.default_params(), j, th0[j] * (1.0 + sgn * 1e-4))
            out.append(orc.Oracle(tables.packed(), params=p).plant_step(x, u, n_sub=4))
        fd[:, :, j] = (out[0] - out[1]) / 2e-4
    assert np.all(ref[4]["dtheta"][:, :, PR.NAMES.index("q_n"):] == 0.0)  # the plant has no cost parameter
    assert np.all(fd[:, :, PR.NAMES.index("q_n"):] == 0.0)
    err = np.abs(S - fd).max(axis=(1, 2)) / np.abs(S).max(axis=(1, 2))
    print(f"max error of the theta columns / max|S theta| = {err.max():.3e}")
    assert err.max() <= 1e-4
