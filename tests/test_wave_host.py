"""CPU: tools/check_wave_host.cpp checks the host-compilable part of csrc/wave.h — hvpr_ord_of strictly monotone with hvpr_of_ord its
inverse over the special values and a few thousand random bit patterns, key 0 below every float, -0.0 and +0.0 apart in the bare map
and together in the score top-k's wrapper (the marked lines of csrc/postprocess.hip, compiled as they stand), hvpr_frame_of around
empty frames — built with the address and undefined-behaviour sanitizers of the host compiler."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ordered_keys_and_frame_of(tmp_path):
    src = open(os.path.join(ROOT, "hvpr_amd", "csrc", "postprocess.hip")).read()
    wrapper = re.search(r"// \[topk_ord\]\n(.*?)// \[/topk_ord\]", src, re.S).group(1)
    assert "hvpr_ord_of" in wrapper
    (tmp_path / "topk_ord.inc").write_text(wrapper)
    exe = str(tmp_path / "check_wave_host")
    # g++, pinned: -static-libasan is its spelling of a statically linked sanitizer runtime
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-static-libasan", "-fno-sanitize-recover=all", "-I", str(tmp_path),
                           os.path.join(ROOT, "tools", "check_wave_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.stdout, r.stderr)
