"""The loop state of `lpgp_pivchol_*` (`csrc/pivchol_state.h`), on the host: a stand-alone program
(`csrc/hosttest/pivchol_state_check.cpp`) built with AddressSanitizer + UBSan and run as a subprocess walks the column coverage of a
row and the state of the loop through tilings in every order (empty pieces included), gaps at the start, in the middle and at the
end, overlaps, pieces out of range (negative, past n, sizes near 2^63), a commit without a pivot, the three stop rules, use after
finish and the borrowers of the factor; every refusal must leave the state as it was.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "linpde-gp_amd", "csrc")


def test_pivchol_state_under_sanitizers(tmp_path):
    gxx = shutil.which(os.environ.get("CXX", "g++"))
    assert gxx is not None, "no host C++ compiler"
    exe = str(tmp_path / "pivchol_state_check")
    # the sanitizer runtimes are linked INTO the program, so that it does not care what else the environment loads before it
    clang = "clang" in subprocess.run([gxx, "--version"], capture_output=True, text=True).stdout
    static_rt = ["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]
    subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    *static_rt, "-Wall", "-Wextra", "-I" + CSRC, os.path.join(CSRC, "hosttest", "pivchol_state_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    res = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    print(res.stdout[-3000:])
    assert res.returncode == 0, res.stdout[-3000:] + "\n" + res.stderr[-4000:]
    assert "pivchol_state_check: all checks passed" in res.stdout
    assert "ERROR: AddressSanitizer" not in res.stderr and "runtime error" not in res.stderr
