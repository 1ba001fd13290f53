"""What `sample` promises without a device: the random-stream contract and the argument checks of `Normal.sample` for scalar
and diagonal covariances (sampled on the host: no arithmetic of the device path, so no device call), the `ValueError`s of the
process-level `sample` that are raised before anything is computed, and the configuration row."""
import numpy as np
import pytest


class _Gen:
    def __init__(self, fn):
        self._fn, self.calls = fn, []

    def standard_normal(self, shape):
        shape = tuple(shape)
        self.calls.append(shape)
        return self._fn(shape)


@pytest.fixture
def no_device(monkeypatch):
    """Any attempt to open a device context fails the test."""
    from linpde_gp_amd import _engine

    def boom(*a, **k):
        raise AssertionError("a host-only sample opened a device context")
    monkeypatch.setattr(_engine, "default_context", boom)
    monkeypatch.setattr(_engine, "Context", boom)


def test_config_row():
    import linpde_gp_amd as lp
    assert lp.config.sample_damping == 1e-6


def test_normal_diagonal_covariance_on_the_host(no_device):
    import linpde_gp_amd as lp
    mean = np.array([1.0, -2.0, 0.5])
    var = np.array([4.0, 0.25, 0.0])
    N = lp.randvars.Normal(mean, var)
    for size, want in (((), ()), (5, (5,)), ((2, 3), (2, 3))):
        g = _Gen(np.random.default_rng(1).standard_normal)
        out = N.sample(g, size=size)
        assert g.calls == [want + (3,)] and out.shape == want + (3,)
        z = np.random.default_rng(1).standard_normal(want + (3,))
        assert np.array_equal(out, mean + np.sqrt(var) * z)
    assert np.array_equal(N.cov_cholesky, np.diag([2.0, 0.5, 0.0]))
    assert N.cov_cholesky is N.cov_cholesky
    # sigma^2 I given as a scalar
    N2 = lp.randvars.Normal(mean, 9.0)
    assert np.array_equal(N2.sample(_Gen(np.ones)), mean + 3.0)


def test_normal_scalar_on_the_host(no_device):
    import linpde_gp_amd as lp
    N = lp.randvars.Normal(1.5, 4.0)
    g = _Gen(np.random.default_rng(2).standard_normal)
    out = N.sample(g, size=(4,))
    assert g.calls == [(4,)] and out.shape == (4,)
    assert np.array_equal(out, 1.5 + 2.0 * np.random.default_rng(2).standard_normal((4,)))
    g = _Gen(np.zeros)
    assert N.sample(g) == 1.5 and g.calls == [()]
    assert N.cov_cholesky == 2.0


def test_normal_value_errors(no_device):
    import linpde_gp_amd as lp
    N = lp.randvars.Normal(np.zeros(2), np.ones(2))
    with pytest.raises(ValueError):
        N.sample(np.random.default_rng(0), size=-1)
    with pytest.raises(ValueError):
        N.sample(_Gen(lambda shape: np.zeros(shape + (1,))))          # a generator that does not honour the requested shape
    with pytest.raises(ValueError):
        lp.randvars.Normal(np.zeros(2), np.array([1.0, -1.0])).sample(np.random.default_rng(0))


def test_process_sample_argument_errors(no_device):
    """Raised before a device is touched: `damping < 0`, a negative `size`, a wrong trailing shape of `x`."""
    import linpde_gp_amd as lp
    cf = lp.randprocs.covfuncs
    prior = lp.GaussianProcess(lp.functions.Zero((2,)), cf.TensorProduct(cf.Matern((), nu=2.5), cf.Matern((), nu=2.5)))
    rng = np.random.default_rng(0)
    x = np.zeros((4, 2))
    with pytest.raises(ValueError):
        prior.sample(rng, x, damping=-1.0)
    with pytest.raises(ValueError):
        prior.sample(rng, x, damping=float("nan"))
    with pytest.raises(ValueError):
        prior.sample(rng, x, size=(2, -1))
    with pytest.raises(ValueError):
        prior.sample(rng, np.zeros((4, 3)))
    # no points: the stream is still consumed once, nothing is computed
    g = _Gen(np.zeros)
    out = prior.sample(g, np.zeros((0, 2)), size=3)
    assert out.shape == (3, 0) and g.calls == [(3, 0)]


def test_out_of_scope_surfaces_say_so():
    import inspect
    from linpde_gp_amd import _spawn
    from linpde_gp_amd.randprocs import _matrix_free
    for cls in (_spawn.RemoteConditionalGaussianProcess, _matrix_free.MatrixFreeConditionalGaussianProcess):
        assert "NotImplementedError" in inspect.getsource(cls.sample)
