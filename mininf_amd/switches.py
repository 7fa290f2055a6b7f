"""
The run-time switches: the ``MININF_AMD_<NAME>`` environment variables, read in one place.

A switch is read when the code it guards runs, never at import and never cached, so a test or a
measurement may set it at any time. This module imports nothing from the package.
"""
import os

# name -> (default, meaning). "0" turns a default-on switch off (anything else, the empty string
# included, leaves it on); "1" turns a default-off switch on (anything else leaves it off).
SWITCHES = {
    "JIT": (True, "compile specialised site programs with hiprtc (fused draws need them); "
                  "also read in C++"),
    "FOLD_PRIOR": (True, "fold a one-element or theta prior site into the launch that reads it"),
    "ABSORB": (True, "the ELBO kernels take over the backward of the guide draws they consume"),
    "FUSE_REDUCE": (True, "finish the site launches' reductions inside the ELBO forward"),
    "BCAST_KSUM": (True, "site launches leave their values summed over the particles"),
    "BETA_SIDE": (True, "a site launch carries the Beta implicit-gradient factors as extra "
                        "workgroups"),
    "FINAL_GRADS": (True, "the ELBO forward writes the guide gradients of a unit upstream"),
    "DEFER_STEP": (True, "hold the step-finishing launch for the optimizer step"),
    "MVN_KERNEL": (True, "native MultivariateNormal log density"),
    "CHOLESKY_KERNEL": (True, "native batched Cholesky factorisation"),
    "LOWRANK_SITE": (True, "native LowRankMultivariateNormal site density and gradients"),
    "DEFER_MATMUL": (True, "leave a model's X @ theta to the linear site kernel"),
    "DEFER_GATHER": (True, "leave a model's alpha[group] to the gathered site kernel"),
    "DEFER_SUM": (True, "leave a model's alpha[group] + X @ theta to the gathered linear site "
                        "kernel (needs DEFER_MATMUL and DEFER_GATHER)"),
    "DEFER_SLOPE": (True, "leave the slope terms beta[group] * x of a model's gathered predictor to "
                          "the gathered slopes site kernel (needs DEFER_GATHER)"),
    "FUSE_ROWS": (True, "a linear launch draws its minibatch's rows itself"),
    "DRAW_IN_LINEAR": (True, "a linear launch draws the guide's theta itself"),
    "BETA_DGRAD": (False, "compute the Beta implicit-gradient factors on a side stream"),
    "FUSE_DRAWS": (True, "Normal guide factors drawn in registers by the site programs"),
    "DEFER_EXP": (True, "leave guide exp transforms to the draws that read them"),
    "DIRECT_GRADS": (True, "write the final guide gradients straight into param.grad"),
}

# Read by other means than enabled(): listed so that every name has one place to be looked up.
ELSEWHERE = {
    "LIB": "path of another build of the library (_native.py; a path, not a switch)",
    "DRAW_PAIRS": "read in C++, not through this module: the fused-draw loop takes two particles "
                  "per iteration (default 0)",
    "ACC_FORM": "read in C++, not through this module: 0 keeps the site programs off their "
                "accumulator form (default on)",
    "JIT_DUMP": "read in C++, not through this module: directory to keep generated sources in",
    "JIT_VERBOSE": "read in C++, not through this module: log each specialised compilation",
    "BCAST_SUFFSTAT": "read in C++, not through this module: the sufficient-statistic floor "
                      "measurement of the broadcast site kernel (default 0)",
    "BCAST_MFMA": "read in C++, not through this module: 0 keeps chunks of 0/1 data off the bf16 "
                  "matrix cores in the broadcast site kernel (default on; BCAST_SUFFSTAT wins)",
    "BCAST_CPW": "read in C++, not through this module: 1, 2 or 4 chunks per workgroup of the "
                 "broadcast site kernel's matrix launch (unset or 0: the smallest that fits one round)",
    "ELBO_EXTERNAL": "read in C++, not through this module: take the large ELBO launch's path at "
                     "any size (tests; default 0)",
    "ELBO_KRED": "named in a comment of csrc/elbo.hip only: no code reads it any more",
    "GROUP_ELBO": "set by tests/test_gpu_final_grads.py: no code reads it any more",
    "LINEAR_ELBO": "set by tests/test_gpu_final_grads.py: no code reads it any more",
}


def enabled(name: str, default: bool = True) -> bool:
    """Whether the switch ``MININF_AMD_<name>`` is on, read from the environment now."""
    if default:
        return os.environ.get("MININF_AMD_" + name, "1") != "0"
    return os.environ.get("MININF_AMD_" + name, "0") == "1"
