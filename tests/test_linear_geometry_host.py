"""
geometry() of tests/linear_reference.py -- the Python restatement of the launch geometry of
csrc/linear.hip that test_gpu_linear_variants.py asserts its kernel variants from -- against the
library's own mi_linear_workspace_bytes, which is host code: for every case of the GPU file and for
a random sweep of shapes. The tile count depends on the stages per block, the LDS combine and the
padded grid, so a drift in any of them changes the byte count. No kernel is launched here.
"""
import ctypes

import numpy as np

from mininf_amd import _native as nat
from tests.linear_reference import geometry, mfma_eligible
from tests.test_gpu_linear_variants import ALL_CASES, FOLDED_PRIOR, MULTI_STAGE, NO_GRADS, PRIORS

BASE = 0x10000   # a dummy non-null, 16-byte aligned address: nothing is dereferenced


def site(N, P, K, family, per_particle, prior, layout, valu, flag_word):
    L = nat.Linear()
    L.K, L.N, L.P = K, N, P
    L.family = family
    L.options = nat.LINEAR_VALU if valu else 0
    L.x = BASE + (4 if layout == "offset1" else 0)
    if layout == "transposed":
        L.x_stride_i, L.x_stride_j = 1, N
    else:
        L.x_stride_i = {"stride40": 40, "stride33": 33}.get(layout, P)
        L.x_stride_j = 1
    L.theta, L.theta_stride_k, L.theta_stride_j = BASE, P, 1
    L.value, L.value_stride_i = BASE, 1
    if per_particle:
        L.scale, L.scale_stride_k = BASE, 1
    else:
        L.scale_constant = 1.0
    L.grad_scale, L.site_scale, L.compute_grads = -1.0, 3.0, 1
    if prior is not None:
        L.prior.present, L.prior.family = 1, prior.family
        L.prior.constant[0], L.prior.constant[1] = prior.c0, prior.c1
        L.prior.scale = prior.scale
        L.prior.flags = ctypes.addressof(flag_word)
    return L


def library_bytes(L):
    size = ctypes.c_size_t()
    assert nat.lib().mi_linear_workspace_bytes(ctypes.byref(L), ctypes.byref(size)) == 0
    return size.value


def test_every_gpu_case_lands_in_its_variant():
    word = ctypes.c_uint32(0)
    assert len(ALL_CASES) > 300
    for case, valu in ALL_CASES:
        g = case.check_variant(valu)
        L = site(case.N, case.P, case.K, case.family, case.per_particle,
                 PRIORS[case.prior] if case.prior else None, case.layout, valu, word)
        assert mfma_eligible(case.P, L.x_stride_i, L.x_stride_j, L.x, valu) == g.mfma, case.id
        assert library_bytes(L) == g.workspace_bytes, (case.id, valu, vars(g))


def test_named_variants_are_all_present():
    """Each variant the GPU file is there for has a case in every family it applies to."""
    for family in (nat.NORMAL, nat.BERNOULLI_LOGITS):
        multi = [c.geometry() for c in MULTI_STAGE if c.family == family]
        assert all(g.mfma and g.stages_per_block >= 2 for g in multi)
        assert {g.pt for g in multi} == {1, 2}
        assert any(g.combine for g in multi) and any(not g.combine for g in multi)
        assert any(g.chunked_finalize for g in multi) and any(not g.chunked_finalize for g in multi)
        assert any(g.empty_row_blocks > 0 for g in multi)
        assert any(g.last_stage_rows == 1 for g in multi)
        assert {g.row_subsets for g in multi} == {1, 2, 4}
        stages = {c.geometry().stages_per_block >= 2 for c in NO_GRADS if c.family == family}
        assert stages == {False, True}
        for prior in PRIORS:
            folded = [c.geometry() for c in FOLDED_PRIOR if c.family == family and c.prior == prior]
            assert {g.stages_per_block >= 2 for g in folded} == {False, True}
    both_tiles = {(c.prior, c.geometry().pt, c.geometry().stages_per_block >= 2) for c in FOLDED_PRIOR}
    assert len(both_tiles) == 3 * 2 * 2


def test_random_shapes_match_the_library():
    rng = np.random.default_rng(20240607)
    word = ctypes.c_uint32(0)
    seen = set()
    for _ in range(200):
        N = int(np.exp(rng.uniform(0, np.log(400000))))
        K = int(np.exp(rng.uniform(0, np.log(20000))))
        P = int(rng.integers(1, 65)) if rng.random() < 0.4 else 4 * int(rng.integers(1, 17))
        family = int(rng.choice([nat.NORMAL, nat.BERNOULLI_LOGITS]))
        per_particle = bool(rng.random() < 0.5)
        prior = PRIORS[str(rng.choice(list(PRIORS)))] if rng.random() < 0.4 else None
        layout = str(rng.choice(["dense", "dense", "dense", "stride40", "stride33", "offset1",
                                 "transposed"]))
        if layout == "stride40" and P > 40:
            layout = "dense"
        valu = bool(rng.random() < 0.15)
        L = site(N, P, K, family, per_particle, prior, layout, valu, word)
        eligible = mfma_eligible(P, L.x_stride_i, L.x_stride_j, L.x, valu)
        g = geometry(N, P, K, per_particle and family == nat.NORMAL, prior is not None, eligible)
        assert library_bytes(L) == g.workspace_bytes, (N, P, K, layout, valu, vars(g))
        supported = ctypes.c_int(-1)
        assert nat.lib().mi_linear_prior_supported(ctypes.byref(L), ctypes.byref(supported)) == 0
        assert supported.value == int(g.mfma)
        seen.add((g.mfma, g.stages_per_block > 1, g.combine, g.chunked_finalize))
    # the sweep reaches both kernels, both stage modes, both partial layouts and both finalizes
    assert {s[0] for s in seen} == {False, True} and {s[1] for s in seen} == {False, True}
    assert {s[2] for s in seen} == {False, True} and {s[3] for s in seen} == {False, True}
