"""The workspace allocator (csrc/workspace.h) without a GPU: tools/workspace_replay.cpp - which includes that header alone - is
built with the address and undefined-behaviour sanitizers and run as a program of its own.  It replays seeded random sequences of
persist / scratch / mark / reset calls dry and real, with the capacity and the scratch base plan_workspace / plan_and_run give the
real pass, and checks that (a) the real pass stays inside its buffer, (b) persist and scratch ranges never meet, (c) one 256-byte
unit less than either peak is reported as an overflow with `base` as the pointer, (d) dry pointers are never inside the buffer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "latent-diffusion-segmentation_amd", "csrc")
SEEDS = ["1", "2", "3", "20240607", "18446744073709551615"]


def test_workspace_header_is_pure_host_code():
    txt = open(os.path.join(CSRC, "workspace.h")).read()
    includes = [l.split()[1] for l in txt.splitlines() if l.startswith("#include")]
    assert includes == ["<array>", "<cstddef>", "<cstdint>"]      # no HIP, no project header
    src = open(os.path.join(ROOT, "tools", "workspace_replay.cpp")).read()
    assert [l.split()[1] for l in src.splitlines() if l.startswith("#include") and '"' in l] == ['"workspace.h"']


def test_workspace_replay_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build tools/workspace_replay.cpp"
    exe = str(tmp_path / "workspace_replay")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "workspace_replay.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe] + SEEDS, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("seed ")]
    assert len(lines) == len(SEEDS) and all(l.endswith(": ok") for l in lines)
