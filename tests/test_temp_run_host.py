"""Host-only checks of the host-free energised run (amc_temp_run_device): the entry points are declared, exported and
bound, the header still compiles as C and as C++ with ABI version 2, and TemperatureSimulation.run keeps its loop without a
device seed.  The argument checks of the entry point need a context, hence a device: tests/test_gpu_temp_run.py has them.

(The small system of that file — n = 2,000, initial conditions of seed 23, 20 steps — was chosen with the CPU oracle:
drift, cases 1-2, wall_hits of the seven cases, sweep, step by step, gives 0 2 2 2 2 1 0 1 1 1 1 1 1 1 1 1 0 0 1 3
energised hits per step with stand-in directions; steps with and without a hit both occur.)"""
import os
import shutil
import subprocess

import pytest

from argon_monte_carlo_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("amc_temp_run_device", "amc_temp_series_read", "amc_set_step")


def test_new_entry_points_are_declared_bound_and_exported():
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "argonmc.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert f"int {name}(amc_ctx *ctx" in hdr, name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    res, args = _lib.SIGNATURES["amc_temp_run_device"]
    assert res is C.c_int and args[1:3] == [C.c_double, C.c_int64] and len(args) == 5
    res, args = _lib.SIGNATURES["amc_temp_series_read"]
    assert args[1:3] == [C.c_int64, C.c_int64] and len(args) == 6
    assert lib.amc_abi_version() == 2


@pytest.mark.parametrize("lang,std", [("c", "-std=c99"), ("c++", "-std=c++11")])
def test_header_compiles_as_c_and_cxx_with_abi_2(tmp_path, lang, std):
    cc = shutil.which("cc" if lang == "c" else "c++")
    if cc is None:
        pytest.skip("no host compiler")
    src = tmp_path / ("t.c" if lang == "c" else "t.cpp")
    src.write_text('#include "argonmc.h"\n'
                   "#if AMC_ABI_VERSION != 2\n#error ABI version\n#endif\n"
                   "int (*run_)(amc_ctx *, double, int64_t, const amc_temp_rng *, amc_step_stats *) = amc_temp_run_device;\n"
                   "int (*read_)(amc_ctx *, int64_t, int64_t, double *, uint8_t *, int64_t *) = amc_temp_series_read;\n"
                   "int (*step_)(amc_ctx *, int64_t) = amc_set_step;\n")
    r = subprocess.run([cc, "-x", lang, std, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                        str(tmp_path / "t.o")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_run_without_a_device_seed_is_still_the_loop_of_timesteps():
    """(no context is built: the method is called on a stand-in that counts the steps)"""
    from argon_monte_carlo_amd.sim import TemperatureSimulation

    class Stub:
        _device_rng = None
        calls = 0

        def timestep(self, dt, collect_paths=True):
            assert collect_paths is False
            self.calls += 1

    s = Stub()
    assert TemperatureSimulation.run(s, 5) is None and s.calls == 5
