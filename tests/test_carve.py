"""CPU test of csrc/carve.h, the cursor every work-space and scratch layout is written with, and of
the resident histogram's scratch layout (csrc/hist_scratch.h).  tests/cpu/carve_main.cpp is a
plain C++ program (the two headers include nothing from HIP) built with the host sanitizers: it
measures layouts with a null base, binds them onto heap blocks of exactly the measured size,
checks alignment, order and bounds, writes every region's first and last byte, and holds the
histogram scratch total to the closed-form expression the layout replaced."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_carve_layouts(tmp_path):
    from aiyagari_hark_amd import build
    exe = str(tmp_path / "carve_main")
    # a host-only compile: the sanitizers instrument the host program and nothing for the GPU
    subprocess.run([build.hipcc(), "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fno-gpu-sanitize", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "cpu", "carve_main.cpp"), "-o", exe], check=True)
    # (a sanitizer report fails the run: ASan exits non-zero, UBSan is told to)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK"
    # the three shapes of the resident histogram's scratch, each equal to the old closed form
    assert [ln.split("=")[0].strip() for ln in lines[:-1]] == [
        "hc_scratch(1, 1, 512)", "hc_scratch(3, 10, 18000)", "hc_scratch(24, 10, 19456)"]
