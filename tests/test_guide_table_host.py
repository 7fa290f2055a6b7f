"""
The guide layer's family table, counters and Philox key helper, as far as a CPU-only host can see
them: a factor a record's ``accepts`` declines keeps torch's entropy, ``guide.counts()`` has the
five keys ``last_fusions`` merges, and ``guide.philox_key`` lays a DrawConfig out in the order in
which every keyed sampler entry point of the C ABI takes it.
"""
import ctypes
import os
import re

import pytest
import torch
from torch.distributions import Dirichlet, Exponential, Laplace, LogNormal, \
    LowRankMultivariateNormal, MultivariateNormal

from mininf_amd import _native as nat, guide

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "mininf_amd.h")
F64 = torch.float64


class _Mvn(MultivariateNormal):
    pass


class _Dirichlet(Dirichlet):
    pass


class _LowRank(LowRankMultivariateNormal):
    pass


class _Exponential(Exponential):
    pass


def _lowrank(D, R, cls=LowRankMultivariateNormal, dtype=torch.float32):
    return cls(torch.zeros(D, dtype=dtype), 0.01 * torch.ones(D, R, dtype=dtype),
               torch.ones(D, dtype=dtype))


# (the record's counter, the variant) -> a factor its ``accepts`` declines: 16 in all. Without a
# device every one of them is host-resident as well; the GPU test draws the accepted ones.
DECLINED = {
    ("mvn", "host"): lambda: MultivariateNormal(torch.zeros(3), scale_tril=torch.eye(3)),
    ("mvn", "double"): lambda: MultivariateNormal(torch.zeros(3, dtype=F64),
                                                  scale_tril=torch.eye(3, dtype=F64)),
    ("mvn", "subclass"): lambda: _Mvn(torch.zeros(3), scale_tril=torch.eye(3)),
    ("mvn", "over MI_MVN_MAX_N"): lambda: MultivariateNormal(
        torch.zeros(nat.MVN_MAX_N + 1), scale_tril=torch.eye(nat.MVN_MAX_N + 1)),
    ("dirichlet", "host"): lambda: Dirichlet(torch.ones(5, 3)),
    ("dirichlet", "double"): lambda: Dirichlet(torch.ones(3, dtype=F64)),
    ("dirichlet", "subclass"): lambda: _Dirichlet(torch.ones(3)),
    ("dirichlet", "over MI_DIRICHLET_MAX_C"): lambda: Dirichlet(
        torch.ones(nat.DIRICHLET_MAX_C + 1)),
    ("lowrank", "host"): lambda: _lowrank(3, 2),
    ("lowrank", "double"): lambda: _lowrank(3, 2, dtype=F64),
    ("lowrank", "subclass"): lambda: _lowrank(3, 2, cls=_LowRank),
    ("lowrank", "over MI_LOWRANK_MAX_R"): lambda: _lowrank(3, nat.LOWRANK_MAX_R + 1),
    ("lowrank", "over MI_LOWRANK_MAX_D"): lambda: _lowrank(nat.LOWRANK_MAX_D + 1, 1),
    ("elementwise", "host"): lambda: Laplace(torch.zeros(5), torch.ones(5)),
    ("elementwise", "double"): lambda: LogNormal(torch.zeros(5, dtype=F64),
                                                 torch.ones(5, dtype=F64)),
    ("elementwise", "subclass"): lambda: _Exponential(torch.ones(5)),
}


def test_table_lists_the_four_families_in_order():
    assert [family.counter for family in guide.FAMILIES] == \
        ["mvn", "dirichlet", "lowrank", "elementwise"]
    assert [family.accepts for family in guide.FAMILIES] == \
        [guide.native_mvn, guide.native_dirichlet, guide.native_lowrank, guide.native_elementwise]
    assert [family.entropy for family in guide.FAMILIES] == \
        [None, guide.dirichlet_entropy, guide.lowrank_entropy, guide.elementwise_entropy]
    assert len(DECLINED) <= 16
    assert {counter for counter, _ in DECLINED} == {family.counter for family in guide.FAMILIES}


@pytest.mark.parametrize("counter,variant", list(DECLINED), ids=lambda x: x.replace(" ", "_"))
def test_declined_factor_keeps_the_torch_entropy(counter, variant):
    factor = DECLINED[counter, variant]()
    (family,) = [family for family in guide.FAMILIES if family.counter == counter]
    assert not family.accepts(factor)
    assert not any(other.accepts(factor) for other in guide.FAMILIES)
    guide.draw_all({}, 4, seed=1, step=0, particle_offset=0)
    assert torch.equal(guide.entropy(factor), factor.entropy().sum())
    assert guide.counts()["lowrank_entropies"] == 0


def test_counts_has_the_five_keys_and_an_empty_guide_draws_nothing():
    assert guide.draw_all({}, 4, seed=1, step=0, particle_offset=0) == {}
    assert guide.counts() == {"mvn_draws": 0, "dirichlet_draws": 0, "lowrank_draws": 0,
                              "elementwise_draws": 0, "lowrank_entropies": 0}
    assert list(guide.counts()) == ["mvn_draws", "dirichlet_draws", "lowrank_draws",
                                    "elementwise_draws", "lowrank_entropies"]


# every sampler entry point that takes the Philox key, and the header's name for the injected noise
KEYED = {"mi_normal_rsample": "eps", "mi_normal_rsample_exp": "eps",
         "mi_normal_rsample_backward": "eps", "mi_beta_rsample": "x_in",
         "mi_beta_rsample_exp": "x_in", "mi_gamma_rsample": "g_in", "mi_mvn_rsample": "eps",
         "mi_mvn_rsample_backward": "eps", "mi_lowrank_rsample": "eps",
         "mi_lowrank_rsample_backward": "eps", "mi_dirichlet_rsample": "g_in",
         "mi_elementwise_rsample": "noise", "mi_elementwise_rsample_backward": "noise"}
KEY_TYPES = {"seed": ctypes.c_uint64, "step": ctypes.c_uint64, "step_device": ctypes.c_void_p,
             "stream_id": ctypes.c_uint32, "particle_offset": ctypes.c_int64,
             "element_offset": ctypes.c_int64, "noise": ctypes.c_void_p}


def _parameter_names(header: str, name: str):
    (arguments,) = re.findall(r"\bint " + name + r"\((.*?)\);", header, flags=re.S)
    return [re.findall(r"\w+", argument)[-1] for argument in arguments.split(",")]


@pytest.mark.parametrize("backward", (False, True), ids=("forward_word", "snapshot"))
def test_key_helper_follows_the_abi_order(backward):
    """A DrawConfig with a distinct value in every field: the helper's tuple, read against the
    parameter names of the header and the types of _native._SIGNATURES, at the position of the key
    in every keyed entry point, with and without element_offset."""
    with open(HEADER) as fh:
        header = fh.read()
    words = torch.zeros(3, dtype=torch.int64)
    noise = torch.zeros(4)
    cfg = guide.DrawConfig(K=7, seed=11, step=12, stream_id=13, particle_offset=14, noise=noise,
                           step_device=words[0:1], step_snapshot=words[1:2], element_offset=16)
    want = {"seed": 11, "step": 12, "stream_id": 13, "particle_offset": 14, "element_offset": 16,
            "step_device": words.data_ptr() + (8 if backward else 0), "noise": noise.data_ptr()}
    assert len(set(want.values())) == len(want)
    with_element = 0
    for name, noise_name in KEYED.items():
        names = _parameter_names(header, name)
        argtypes = nat._SIGNATURES[name][1]
        assert len(names) == len(argtypes), name
        first = names.index("seed")
        element = "element_offset" in names
        with_element += element
        key = guide.philox_key(cfg, backward=backward, element=element)
        fields = [noise_name if field == "noise" else field for field in
                  ("seed", "step", "step_device", "stream_id", "particle_offset",
                   *(("element_offset",) if element else ()), "noise")]
        assert names[first:first + len(key)] == fields, name
        assert list(argtypes[first:first + len(key)]) == \
            [KEY_TYPES["noise" if field == noise_name else field] for field in fields], name
        assert list(key) == [want["noise" if field == noise_name else field]
                             for field in fields], name
    assert with_element == 3   # the Normal entry points alone
    # no snapshot: the backward reads the forward's word; no noise, no word: null
    bare = guide.DrawConfig(K=7, seed=-1, step=1 << 64, stream_id=13, particle_offset=14)
    assert guide.philox_key(bare, backward=backward) == ((1 << 64) - 1, 0, None, 13, 14, None)
    bare.step_device = words[2:3]
    assert guide.philox_key(bare, backward=backward)[2] == words.data_ptr() + 16
