"""The index rule of the heard form's full-lane record copies (rm_device.hpp: kCopySpan, run_of, run_place)
in a stand-alone program under the host sanitizers: tests/cpp/wave_runs_san_test.cpp replays the wave's walk over random and adversarial length vectors of 64 runs and holds it to a plain expansion of the runs.  Host code only: the program has
its own main and touches no device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_index_rule_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "wave_runs_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-I" + csrc, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "wave_runs_san_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
