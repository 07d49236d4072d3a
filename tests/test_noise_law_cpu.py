"""CPU checks of the uniform noise law (CGPT_NOISE_UNIFORM): the L1 certificate of the *_law statistics, the Gaussian
delegations left bit-identical, bad laws rejected by every new entry point, and the Smooth constructor's law checks."""
import ctypes as C

import numpy as np
import pytest

import certifiedgpt_amd as cg
from certifiedgpt_amd import _lib
from oracle import smooth_oracle as so

GAUSSIAN, UNIFORM = 0, 1


def _many(L, table, n, alpha, scale, law=None):
    t = np.ascontiguousarray(table, dtype=np.int64)
    G, K = t.shape[0], t.shape[2]
    labels, radii = np.empty(G, dtype=np.int32), np.empty(G, dtype=np.float64)
    p = (t.ctypes.data_as(C.c_void_p), G, K, n, alpha, scale)
    out = (labels.ctypes.data_as(C.c_void_p), radii.ctypes.data_as(C.c_void_p))
    st = L.cgpt_certify_many_from_counts(*p, *out) if law is None else L.cgpt_certify_many_from_counts_law(*p, law, *out)
    assert st == 0, L.cgpt_last_error()
    return labels, radii


def _random_tables(rng, trials):
    """(table [G,2,K], n, alpha, scale) with nA spread over the whole range, abstentions and sure wins included."""
    for _ in range(trials):
        G, K = int(rng.integers(1, 9)), int(rng.integers(2, 12))
        n = int(rng.choice([1, 2, 10, 100, 1000, 100000]))
        alpha = float(rng.choice([0.001, 0.01, 0.05, 0.3]))
        scale = float(rng.uniform(0.01, 4.0))
        n0 = int(rng.integers(1, 200))
        t = np.zeros((G, 2, K), dtype=np.int64)
        for g in range(G):
            t[g, 0] = rng.multinomial(n0, rng.dirichlet(np.full(K, 0.3)))
            t[g, 1] = rng.multinomial(n, rng.dirichlet(np.full(K, 0.3)))
        yield t, n, alpha, scale


def test_uniform_radius_is_scale_times_margin_over_one_half():
    L = cg.lib()
    rng = np.random.default_rng(20261016)
    certified = abstained = 0
    for t, n, alpha, scale in _random_tables(rng, 300):
        lab_u, rad_u = _many(L, t, n, alpha, scale, UNIFORM)
        lab_g, _ = _many(L, t, n, alpha, scale, GAUSSIAN)
        assert lab_u.tolist() == lab_g.tolist()                       # the law changes the radius only
        for g in range(t.shape[0]):
            cA = int(np.argmax(t[g, 0]))
            nA = int(t[g, 1, cA])
            p = L.cgpt_lower_confidence_bound(nA, n, alpha)
            if p < 0.5:
                assert (lab_u[g], rad_u[g]) == (-1, 0.0)
                abstained += 1
                continue
            certified += 1
            assert lab_u[g] == cA
            assert rad_u[g] == scale * (p - 0.5)                      # the same float64 expression, bit for bit
            assert abs(rad_u[g] - scale * (so.lower_confidence_bound(nA, n, alpha) - 0.5)) <= 1e-9
    assert certified > 100 and abstained > 20, (certified, abstained)


def test_uniform_abstains_exactly_below_one_half_and_certifies_zero_at_the_boundary():
    L = cg.lib()
    # nA = n = 1 at alpha = 1/2: the Clopper-Pearson bound is alpha^(1/n) = 0.5 exactly -> certified, radius 0
    assert L.cgpt_lower_confidence_bound(1, 1, 0.5) == 0.5
    lab, rad = _many(L, [[[0, 1], [0, 1]]], 1, 0.5, 2.0, UNIFORM)
    assert (lab[0], rad[0]) == (1, 0.0)
    # just below: nA = 1 of n = 1 at alpha = 0.49 -> p = 0.49 < 1/2 -> abstain
    lab, rad = _many(L, [[[0, 1], [0, 1]]], 1, 0.49, 2.0, UNIFORM)
    assert (lab[0], rad[0]) == (-1, 0.0)
    # nA = 0: bound 0 -> abstain under both laws
    for law in (GAUSSIAN, UNIFORM):
        lab, rad = _many(L, [[[5, 0], [0, 9]]], 9, 0.05, 1.0, law)
        assert (lab[0], rad[0]) == (-1, 0.0)


def test_gaussian_law_is_bit_identical_to_the_existing_functions():
    L = cg.lib()
    rng = np.random.default_rng(7)
    for t, n, alpha, scale in _random_tables(rng, 150):
        lab_l, rad_l = _many(L, t, n, alpha, scale, GAUSSIAN)
        lab_m, rad_m = _many(L, t, n, alpha, scale)
        assert lab_l.tolist() == lab_m.tolist() and rad_l.tobytes() == rad_m.tobytes()
        for g in range(t.shape[0]):
            cs, ce = np.ascontiguousarray(t[g, 0]), np.ascontiguousarray(t[g, 1])
            lab, rad = C.c_int32(), C.c_double()
            assert L.cgpt_certify_from_counts(cs.ctypes.data_as(C.c_void_p), ce.ctypes.data_as(C.c_void_p), t.shape[2], n, alpha,
                                              scale, C.byref(lab), C.byref(rad)) == 0
            assert lab.value == lab_l[g] and np.float64(rad.value).tobytes() == rad_l[g].tobytes()


@pytest.mark.parametrize("law", [-1, 2, 7, 1 << 30])
def test_bad_law_is_rejected_by_every_new_entry_point(law):
    L = cg.lib()
    t = np.zeros((1, 2, 3), dtype=np.int64)
    labels, radii = np.empty(1, dtype=np.int32), np.empty(1, dtype=np.float64)
    dummy = C.c_void_p(0x1000)          # never dereferenced: the law is checked before anything else
    calls = {
        "cgpt_set_noise_law": lambda: L.cgpt_set_noise_law(dummy, law),
        "cgpt_noise_batch_law": lambda: L.cgpt_noise_batch_law(dummy, 12, 0, 1, 0.5, law, 0, dummy, None),
        "cgpt_certify_many_from_counts_law": lambda: L.cgpt_certify_many_from_counts_law(
            t.ctypes.data_as(C.c_void_p), 1, 3, 10, 0.05, 0.5, law, labels.ctypes.data_as(C.c_void_p), radii.ctypes.data_as(C.c_void_p)),
        "cgpt_certify_device_law": lambda: L.cgpt_certify_device_law(dummy, dummy, 3, 10, 0.05, 0.5, law, dummy, None),
    }
    for name, call in calls.items():
        assert call() == 1, name                                    # CGPT_ERR_INVALID
        assert b"law" in L.cgpt_last_error(), (name, L.cgpt_last_error())


def test_new_symbols_are_bound():
    for name in ("cgpt_set_noise_law", "cgpt_noise_batch_law", "cgpt_certify_many_from_counts_law", "cgpt_certify_device_law"):
        assert name in _lib.SIGNATURES and hasattr(cg.lib(), name)


class _GaussianOnlyEngine:
    """A duck-typed engine that predates the law keyword."""

    def sample_counts(self, x, first_sample, num, batch_size, sigma, seed, counts=None):
        raise AssertionError("not called in these tests")

    def eval(self):
        return self


def test_smooth_constructor_checks_the_law():
    s = cg.Smooth(lambda b: b, 3, 0.5)
    assert s.norm == "l2" and s.noise == "gaussian"
    s = cg.Smooth(lambda b: b, 3, 0.5, noise="uniform")               # a plain callable takes the generic path: both laws
    assert s.norm == "l1" and s.noise == "uniform"
    with pytest.raises(ValueError):
        cg.Smooth(lambda b: b, 3, 0.5, noise="laplace")
    with pytest.raises(ValueError):
        cg.Smooth(lambda b: b, 3, 0.5, noise="Uniform")
    # an engine must list the law; one that lists nothing is Gaussian-only and keeps working as such
    with pytest.raises(ValueError):
        cg.Smooth(_GaussianOnlyEngine(), 3, 0.5, noise="uniform")
    assert cg.Smooth(_GaussianOnlyEngine(), 3, 0.5).norm == "l2"
    eng = _GaussianOnlyEngine()
    eng.noise_laws = ("gaussian", "uniform")
    assert cg.Smooth(eng, 3, 0.5, noise="uniform").norm == "l1"
    with pytest.raises(AttributeError):
        cg.Smooth(eng, 3, 0.5).norm = "l1"                           # read-only


def test_smooth_certifies_l1_radii_from_counts():
    rng = np.random.default_rng(3)
    sg = cg.Smooth(lambda b: b, 6, 0.75)
    su = cg.Smooth(lambda b: b, 6, 0.75, noise="uniform")
    for t, n, alpha, _ in _random_tables(rng, 40):
        t = t[:, :, :6] if t.shape[2] >= 6 else np.pad(t, ((0, 0), (0, 0), (0, 6 - t.shape[2])))
        many = su.certify_many_from_counts(t, n, alpha)
        for g in range(t.shape[0]):
            lab_g, _ = sg.certify_from_counts(t[g, 0], t[g, 1], n, alpha)
            lab_u, rad_u = su.certify_from_counts(t[g, 0], t[g, 1], n, alpha)
            assert (lab_u, rad_u) == many[g]
            assert lab_u == lab_g
            if lab_u == -1:
                assert rad_u == 0.0
            else:
                nA = int(t[g, 1, int(np.argmax(t[g, 0]))])
                assert abs(rad_u - 0.75 * (so.lower_confidence_bound(nA, n, alpha) - 0.5)) <= 1e-9
        assert sg.certify_many_from_counts(t, n, alpha) == [sg.certify_from_counts(t[g, 0], t[g, 1], n, alpha) for g in range(t.shape[0])]


def test_noise_batch_rejects_an_unknown_law_before_touching_the_device():
    from certifiedgpt_amd.classifier import noise_batch
    with pytest.raises(ValueError):
        noise_batch(None, 0, 1, 0.5, 0, law="laplace")
