"""The sampling layer is one module per concern; ``linna_amd.sampler`` keeps the drivers and re-exports every name it used to
define (functions and classes, public and private) as the identical object of its home module.  The import test starts its
four child processes side by side, so it costs one import of torch (about 3 s), not four."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every function and class sampler.py defined at module level before the split, and where it lives now
HOME = {
    "chainstats": ["_next_pow_two", "_autocorr_1d", "integrated_time", "_chain3", "split_rhat", "_ndtri", "_rank2", "_rhat_of_scores",
                   "rank_rhat", "multichain_ess", "DeviceChain", "checkmeanstd"],
    "chainstore": ["_OnDisk", "ChainStore", "get_good_walker_list", "read_chain_and_cut"],
    "ensemble": ["EnsembleSampler", "_FastOverflow", "SliceEnsembleSampler"],
    "hmc": ["BatchedHMC"],
    "sampler": ["_Ranks", "_Prof", "_run_blocks", "HMCSampler", "ZeusSampler"],
}
ALL = ["EnsembleSampler", "SliceEnsembleSampler", "BatchedHMC", "HMCSampler", "ZeusSampler", "checkmeanstd", "integrated_time",
       "split_rhat", "multichain_ess", "ChainStore", "DeviceChain", "read_chain_and_cut", "get_good_walker_list"]


def test_sampler_reexports_every_name_from_its_home_module():
    pytest.importorskip("torch")
    import importlib
    from linna_amd import sampler
    assert sum(len(v) for v in HOME.values()) == 25
    for module, names in HOME.items():
        home = importlib.import_module("linna_amd." + module)
        for name in names:
            assert getattr(sampler, name) is getattr(home, name), name
            assert getattr(home, name).__module__ == "linna_amd." + module, name
    assert sampler.__all__ == ALL
    assert all(hasattr(sampler, name) for name in sampler.__all__)


def test_the_new_modules_import_without_the_drivers():
    pytest.importorskip("torch")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    code = "import linna_amd.%s, sys; assert 'linna_amd.sampler' not in sys.modules, 'a module below the drivers imports them'"
    children = {m: subprocess.Popen([sys.executable, "-c", code % m], env=env, cwd=ROOT, stderr=subprocess.PIPE, text=True)
                for m in ("chainstats", "chainstore", "ensemble", "hmc")}       # (side by side: the cost is one import of torch)
    for m, child in children.items():
        err = child.communicate()[1]
        assert child.returncode == 0, (m, err[-2000:])
