"""The host logic of the shared heard-form cache (rm_ncpool.hpp) in a stand-alone program under the host
sanitizers: tests/cpp/ncpool_host_san_test.cpp packs and unpacks the 64-bit entry at its field limits, and drives the registry's
key, attach, detach and epoch rule from several host threads -- reference counts, "the last context frees", "never a new epoch
while shared".  Host code only: the program has its own main and touches no device."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_rules_under_sanitizers(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    csrc = os.path.join(ROOT, "radio-sim_amd", "csrc")
    exe = os.path.join(str(tmp_path), "ncpool_host_san_test")
    subprocess.check_call([hipcc, "-O1", "-g", "-std=c++17", "-pthread", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                           "-I" + csrc, "-x", "hip", os.path.join(ROOT, "tests", "cpp", "ncpool_host_san_test.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().splitlines()[-1] == "ok", (p.returncode, p.stdout, p.stderr)
    assert "runtime error" not in p.stderr, p.stderr    # (the undefined-behaviour sanitizer reports and goes on)
