"""Which kernels of the library does the non-GPU suite launch?  Every test module runs in a pytest process of its own with the
emulator's launch log on (JSS_EMU_LAUNCH_LOG, launches executed: tests/emu/hip/hip_runtime.h opens the log once per process),
and the 'launch <kernel> ...' lines are counted per kernel.  The list of kernels is read from the built emulator library
(tests/kernel_matrix_cases.py: library_kernels), so a kernel nothing launches is listed with a count of 0.

usage: python tools/kernel_coverage.py OUT.txt [-j N] [tests/test_x.py ...]        (default: every tests/test_*.py)
Recorded runs: profiles/r13_kernel_matrix/."""
import argparse
import collections
import concurrent.futures
import glob
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "emu"), ROOT]


def run_module(module, log):
    env = dict(os.environ, JSS_EMU_LAUNCH_LOG=log)
    env.pop("JSS_EMU_LAUNCH_DRY", None)
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", module], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    tail = (r.stdout.strip().splitlines() or ["?"])[-1]
    return module, time.time() - t0, r.returncode, tail


def count_launches(log):
    from kernel_matrix_cases import short_name
    counts = collections.Counter()
    if os.path.isfile(log):
        with open(log) as f:
            for line in f:
                if line.startswith("launch "):
                    counts[short_name(line[len("launch "):].rsplit(" grid=", 1)[0])] += 1
    return counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--base", help="a tally this tool wrote for the OTHER modules of the suite: its counts are added, its "
                                   "module lines kept, so that a run of the new modules alone gives the tally of the whole suite")
    ap.add_argument("modules", nargs="*")
    a = ap.parse_intermixed_args()
    from emu_backend import build as build_emu
    from kernel_matrix_cases import library_kernels
    kernels = library_kernels(build_emu())
    modules = a.modules or sorted(os.path.relpath(p, ROOT) for p in glob.glob(os.path.join(ROOT, "tests", "test_*.py")))
    total, per_module, rows, base_by, base_lines = collections.Counter(), {}, [], {}, []
    if a.base:
        with open(a.base) as f:
            for line in f:
                if line.startswith("# tests/"):
                    base_lines.append(line)
                elif not line.startswith("#"):
                    count, name = line.split(None, 1)
                    name, _, by = name.strip().partition("   (")
                    total[name] += int(count)
                    base_by[name] = [m for m in by.rstrip(")").split(", ") if m]
    t0 = time.time()
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(a.j) as pool:
        logs = {m: os.path.join(tmp, os.path.basename(m) + ".log") for m in modules}
        for m, secs, rc, tail in pool.map(lambda m: run_module(m, logs[m]), modules):
            per_module[m] = count_launches(logs[m])
            total.update(per_module[m])
            rows.append((m, secs, rc, tail))
            print(f"{m}: {secs:.0f} s, exit {rc}, {tail}", flush=True)
    wall = time.time() - t0
    unknown = sorted(set(total) - set(kernels))
    assert not unknown, f"launched, but not a kernel symbol of the library: {unknown}"
    reached = [k for k in kernels if total[k]]
    with open(a.out, "w") as f:
        f.write(f"# python tools/kernel_coverage.py: launches per kernel of the emulator library, launches executed\n")
        f.write(f"# {len(reached)} of {len(kernels)} kernels launched; {len(modules)} modules, {a.j} at a time, "
                f"{wall:.0f} s wall, {sum(r[1] for r in rows):.0f} s summed over the modules\n")
        if a.base:
            f.write(f"# the modules of {os.path.relpath(a.base, ROOT)} are not run again: their counts are added, their lines follow\n")
            f.writelines(base_lines)
        for m, secs, rc, tail in rows:
            f.write(f"# {m}: {secs:.0f} s, exit {rc}, {sum(per_module[m].values())} launches of "
                    f"{sum(1 for k in kernels if per_module[m][k])} kernels; {tail}\n")
        f.write("# launches  kernel   (modules that launch it)\n")
        for k in kernels:
            by = base_by.get(k, []) + [os.path.basename(m)[5:-3] for m in modules if per_module[m][k]]
            f.write(f"{total[k]:9d}  {k}" + (f"   ({', '.join(by)})" if by else "") + "\n")
    print(f"{len(reached)} of {len(kernels)} kernels launched -> {a.out}")


if __name__ == "__main__":
    main()
