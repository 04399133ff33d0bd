"""CPU: tools/check_wino_walk.cpp replays the Winograd kernel's tile walk (csrc/wino_walk.h, paired ragged edge tiles) on the host
for all H, W in 1..80 and N in 1..3 — every (image, tile, channel tile) exactly once — built with the address and undefined-behaviour
sanitizers of the host compiler."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_produces_every_tile_once(tmp_path):
    exe = str(tmp_path / "check_wino_walk")
    # g++, pinned: -static-libasan is its spelling of a statically linked sanitizer runtime
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-static-libasan", "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "check_wino_walk.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.startswith("ok:"), (r.stdout, r.stderr)
