"""The launches of the HIP library's host code are pinned: which kernel instantiation, grid, block, dynamic LDS bytes and
stream every entry point launches with, and which events it records and waits for, over a fixed list of calls
(tests/launch_log_calls.py: every launching entry point, the four kernel shapes, the table and record layouts, sub-batches
that fill, part-fill and overfill n_sub, fork/join on and off, zero-step windows, fused and unfused multi-set calls, batches
on both sides of the two-envs-per-wavefront threshold).  The emulator build compiles that host code unchanged; its launch
log (tests/emu/hip/hip_runtime.h, JSS_EMU_LAUNCH_LOG) is compared with the one recorded in tests/golden/launch_log.txt.
Host-only: nothing is executed, no GPU is needed."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "launch_log.txt")
sys.path[:0] = [os.path.join(HERE, "emu"), os.path.dirname(HERE)]


def record(path):
    """Runs the call list in a fresh process (the library's event registry and the log's event numbers start from nothing)."""
    from emu_backend import build as build_emu
    if os.path.exists(path):
        os.remove(path)
    env = dict(os.environ, JSS_EMU_LAUNCH_LOG=path, JSS_EMU_LAUNCH_DRY="1")
    subprocess.check_call([sys.executable, os.path.join(HERE, "launch_log_calls.py"), build_emu(), path], env=env)
    with open(path) as f:
        return f.read().splitlines()


def by_call(lines):
    calls, name = {}, None
    for line in lines:
        if line.startswith("# "):
            name = line[2:]
            assert name not in calls, f"call listed twice: {name}"
            calls[name] = []
        else:
            calls[name].append(line)
    return calls


def test_launches_match_the_recorded_log(tmp_path):
    got = by_call(record(str(tmp_path / "launch_log.txt")))
    with open(GOLDEN) as f:
        want = by_call(f.read().splitlines())
    assert list(got) == list(want), "the list of calls changed: record the log again (python tests/test_launch_log.py)"
    differ = [name for name in want if got[name] != want[name]]
    for name in differ[:5]:
        print(f"--- {name}\nrecorded:\n  " + "\n  ".join(want[name]) + "\nnow:\n  " + "\n  ".join(got[name]))
    assert not differ, f"{len(differ)} of {len(want)} calls launch differently, the first: {differ[0]}"
    launches = [line for lines in want.values() for line in lines if line.startswith("launch ")]
    assert len(launches) > 1000 and not any(" ? " in line for line in launches)      # (every kernel has its name)


if __name__ == "__main__":           # python tests/test_launch_log.py: records tests/golden/launch_log.txt anew
    print(len(record(GOLDEN)), "lines ->", GOLDEN)
