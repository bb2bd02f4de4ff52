"""The fixed list of C-ABI calls behind tests/test_launch_log.py, run as a script in a process of its own:

    JSS_EMU_LAUNCH_LOG=<file> JSS_EMU_LAUNCH_DRY=1 python tests/launch_log_calls.py <emulator library> <file>

Every call goes to the emulator library (the HIP library's host code compiled unchanged), which logs each kernel launch,
event record and stream wait and -- dry -- executes none of them: the descriptors carry made-up addresses, full-size
batches cost nothing.  This script adds a '# <call> -> <return code>' line in front of what each call logged.  Streams are
the small integers 1..16, so the log says which of a call's streams a launch went to."""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from jssenv_amd import _abi  # noqa: E402

NF, NFC, NFM = 0, _abi.NFC, _abi.NFM          # JssDesc.record_ints (0: full records)
FIFO, MWR = _abi.POLICY["FIFO"], _abi.POLICY["MWR"]
FORK = _abi.ROLLOUT_FORK_JOIN
STREAMS = (C.c_void_p * 16)(*range(1, 17))
STREAM = 1

# (jobs, machines): 16-lane groups, 32-lane groups, one wavefront per env with one job per lane, with two jobs per lane
SHAPES = {"p16": (10, 10), "p32": (20, 15), "w1": (50, 20), "w2": (100, 20)}
# instance tables x job records
LAYOUTS = {"shared-full": ("shared", NF), "shared-compact": ("shared", NFC), "map-full": ("map", NF),
           "own-full": ("own", NF), "own-medium": ("own", NFM)}

_next = [0x10000000000]


def ptr():
    """A made-up device address, 4 KiB aligned, 64 GiB from the next one."""
    _next[0] += 1 << 36
    return _next[0]


def desc(batch, shape, layout, **kw):
    (J, M), (tables, records) = SHAPES[shape] if isinstance(shape, str) else shape, LAYOUTS[layout]
    d = _abi.JssDesc(batch=batch, jmax=J, mmax=M, n_tables={"shared": 1, "map": 3, "own": batch or 1}[tables], ops=ptr(), rem=ptr(),
                     inst=ptr(), table_of_env=ptr() if tables == "map" else None, record_ints=records)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def state():
    return _abi.JssState(*(ptr() for _ in range(6)))


def out():
    return _abi.JssOut(*(ptr() for _ in range(5)))


def arr(typ, items):
    P = C.POINTER(typ)
    return (P * len(items))(*[C.pointer(x) for x in items])


def sets(descs):
    n = len(descs)
    return n, arr(_abi.JssDesc, descs), arr(_abi.JssState, [state() for _ in descs]), arr(_abi.JssOut, [out() for _ in descs])


def ptrs(n):
    return (C.c_void_p * n)(*[ptr() for _ in range(n)])


def calls(lib, search):
    """Yields (name, thunk)."""
    byref = C.byref
    for shape in SHAPES:
        for layout in LAYOUTS:
            for batch in (1000,) + ((20479, 20480, 65536) if (shape, layout) in (("w1", "own-full"), ("w1", "own-medium"),
                                                                                  ("p16", "own-full")) else ()):
                tag = f"{shape}/{layout}/b{batch}"
                d, s, o = desc(batch, shape, layout), state(), out()
                yield f"reset {tag}", lambda d=d, s=s, o=o: lib.jss_reset(byref(d), byref(s), byref(o), None, STREAM)
                yield f"step {tag}", lambda d=d, s=s, o=o: lib.jss_step(byref(d), byref(s), ptr(), byref(o), STREAM)
                yield f"step_autoreset {tag}", lambda d=d, s=s, o=o: lib.jss_step_autoreset(byref(d), byref(s), ptr(), byref(o), STREAM)
                lg = _abi.JssLogits(logits=ptr(), row=0, dtype=_abi.LOGITS_F32, temperature=1.0, action=ptr(), logp=ptr(),
                                    entropy=ptr())
                yield f"step_logits {tag}", lambda d=d, s=s, o=o, lg=lg: lib.jss_step_logits(byref(d), byref(s), byref(lg), 7, 0, byref(o), STREAM)
                yield f"advance {tag}", lambda d=d, s=s, o=o: lib.jss_advance(byref(d), byref(s), None, ptr(), byref(o), STREAM)
                yield f"policy {tag}", lambda d=d, s=s: lib.jss_policy(byref(d), byref(s), MWR, 7, 0, ptr(), STREAM)
                for n_iter in (1, 5):
                    yield f"rollout n_iter={n_iter} {tag}", lambda d=d, s=s, o=o, n=n_iter: lib.jss_rollout(
                        byref(d), byref(s), byref(o), FIFO, 7, 0, n, 0, STREAM)
                tr = _abi.JssTraj(ptr(), ptr(), ptr(), ptr(), ptr(), 0)
                yield f"trajectory {tag}", lambda d=d, s=s, o=o, tr=tr: lib.jss_trajectory(byref(d), byref(s), byref(o), byref(tr), FIFO, 7, 0, 4, 0, STREAM)
                for n in (0, 4):
                    yield f"steps n_steps={n} {tag}", lambda d=d, s=s, o=o, tr=tr, n=n: lib.jss_steps(
                        byref(d), byref(s), byref(o), byref(tr), ptr(), n, STREAM)
                la = _abi.JssLookahead(n=777, parent=ptr(), action=ptr(), id_base=0, makespan=ptr(), steps=ptr(), reward_num=ptr())
                yield f"lookahead {tag}", lambda d=d, s=s, la=la: search.jss_lookahead(byref(d), byref(s), byref(la), FIFO, 7, 0, 0, STREAM)
    # kernel-flavour bits of JssDesc, a shape class inside wider rows, a batch too large for the packed lookahead's lane offsets
    for name, kw in (("wave", {"kernel": 1}), ("auto-1env", {"kernel": 2}), ("wave-2env", {"kernel": 5})):
        for shape, batch in (("p16", 1000), ("w1", 1000), ("w1", 65536)):
            d, s, o = desc(batch, shape, "own-full", **kw), state(), out()
            yield f"step kernel={name} {shape}/b{batch}", lambda d=d, s=s, o=o: lib.jss_step(byref(d), byref(s), ptr(), byref(o), STREAM)
            yield f"rollout kernel={name} {shape}/b{batch}", lambda d=d, s=s, o=o: lib.jss_rollout(byref(d), byref(s), byref(o), FIFO, 7, 0, 1, 0, STREAM)
    d, s, o = desc(1000, (100, 20), "own-full", jclass=50, mclass=20), state(), out()
    yield "step class 50x20 in 100x20", lambda d=d, s=s, o=o: lib.jss_step(byref(d), byref(s), ptr(), byref(o), STREAM)
    d, s = desc(3000000, "p32", "own-full"), state()
    la = _abi.JssLookahead(n=777, parent=ptr(), action=ptr(), id_base=0, makespan=ptr(), steps=ptr(), reward_num=ptr())
    yield "lookahead p32/own-full/b3000000", lambda d=d, s=s, la=la: search.jss_lookahead(byref(d), byref(s), byref(la), FIFO, 7, 0, 0, STREAM)
    la0 = _abi.JssLookahead(n=0, parent=ptr(), action=ptr(), id_base=0, makespan=ptr(), steps=ptr(), reward_num=ptr())
    yield "lookahead n=0", lambda d=d, s=s, la=la0: search.jss_lookahead(byref(d), byref(s), byref(la), FIFO, 7, 0, 0, STREAM)

    # ---- windows of steps over sub-batches on streams: one set -------------------------------------------------------------
    # (batch 100 with n_sub 16: two parts of 64 and 36 envs, fourteen dropped; 30 000 envs in two parts: the whole batch is
    #  above the two-envs-per-wavefront threshold of 20 480, a part below; 65 536 in three: both above)
    windows = [(shape, layout, 1000, n_sub, flags, 3) for shape, layout in (("p16", "shared-compact"), ("p32", "own-medium"),
                                                                           ("w1", "map-full"), ("w2", "own-full"))
               for n_sub in (1, 2, 3) for flags in (0, FORK)]
    windows += [("w1", "own-full", 100, 16, FORK, 2), ("w1", "own-full", 100, 16, 0, 2), ("p16", "own-full", 64, 2, FORK, 2),
                ("w1", "own-full", 30000, 2, FORK, 2), ("w1", "own-medium", 30000, 2, 0, 2), ("w1", "own-full", 30000, 1, FORK, 2),
                ("w1", "own-full", 65536, 3, FORK, 2), ("w1", "own-full", 65536, 4, FORK, 1), ("p32", "own-full", 65536, 3, FORK, 2),
                ("w1", "own-full", 1000, 3, FORK, 0), ("w1", "own-full", 1000, 3, FORK | _abi.ROLLOUT_AUTORESET, 1),
                ("w1", "own-full", 0, 2, FORK, 2)]
    for shape, layout, batch, n_sub, flags, n_steps in windows:
        tag = f"{shape}/{layout}/b{batch} n_sub={n_sub} flags={flags} n_steps={n_steps}"
        d, s, o = desc(batch, shape, layout), state(), out()
        yield f"rollout_steps {tag}", lambda d=d, s=s, o=o, a=(n_steps, flags, n_sub): lib.jss_rollout_steps(
            byref(d), byref(s), byref(o), FIFO, 7, 0, *a, STREAMS)
        yield f"policy_step_steps {tag}", lambda d=d, s=s, o=o, a=(n_steps, flags, n_sub): lib.jss_policy_step_steps(
            byref(d), byref(s), byref(o), MWR, 7, 0, ptr(), *a, STREAMS)

    # ---- several sets ------------------------------------------------------------------------------------------------
    fused = [("p16", "own-full", 3000), ("p32", "own-medium", 2000), ("w1", "own-full", 1500), ("w2", "own-full", 700)]
    combos = {
        "fused4": fused,
        "fused2-reversed": [fused[3], fused[0]],
        "fused6-same-flavour": fused + [("p16", "own-full", 100), ("w1", "map-full", 64)],
        "one-set": fused[:1],
        "with-shared-table": fused[:2] + [("w1", "shared-full", 500)],
        "seven-sets": fused + fused[:3],
        "medium-wave": [("w1", "own-medium", 30000), ("p16", "own-full", 1000)],     # (no medium body on the wave shapes)
        "big-fused": [("w1", "own-full", 30000), ("p16", "own-full", 65536)],
        "ragged-parts": [("w1", "own-full", 1000), ("p16", "own-full", 100), ("p32", "own-full", 0)],
    }
    for name, combo in combos.items():
        ds = [desc(b, shape, layout) for shape, layout, b in combo]
        n, D, S, O = sets(ds)
        yield f"multi_reset {name}", lambda a=(n, D, S, O): lib.jss_multi_reset(*a, None, STREAM)
        yield f"multi_step {name}", lambda a=(n, D, S), O=O: lib.jss_multi_step(*a, ptrs(n), O, 1, STREAM)
        lgs = arr(_abi.JssLogits, [_abi.JssLogits(logits=ptr(), row=0, dtype=_abi.LOGITS_BF16, temperature=1.0, action=ptr(),
                                                  logp=ptr(), entropy=ptr()) for _ in ds])
        yield f"multi_step_logits {name}", lambda a=(n, D, S, lgs), O=O: lib.jss_multi_step_logits(*a, 7, 0, O, STREAM)
        yield f"multi_policy {name}", lambda a=(n, D, S): lib.jss_multi_policy(*a, MWR, 7, 0, ptrs(n), STREAM)
        for n_sub, flags, n_steps in ((1, 0, 2), (1, FORK, 2), (2, 0, 2), (2, FORK, 2), (3, FORK, 2), (8, FORK, 1), (16, 0, 1),
                                      (3, FORK, 0)):
            yield f"multi_rollout {name} n_sub={n_sub} flags={flags} n_steps={n_steps}", lambda a=(n, D, S, O), b=(
                n_steps, flags, n_sub): lib.jss_multi_rollout(*a, FIFO, 7, 0, *b, STREAMS)
        for flags, n_steps in ((0, 2), (FORK, 2), (FORK, 0)):
            yield f"rollout_steps_multi {name} flags={flags} n_steps={n_steps}", lambda a=(n, D, S, O), b=(
                n_steps, flags): lib.jss_rollout_steps_multi(*a, FIFO, 7, 0, *b, STREAMS)
    # a class inside padded rows in the fused grid (full records), and one the grid has no body for (medium records)
    for name, layout in (("fused-classes", "own-full"), ("unfused-classes", "own-medium")):
        ds = [desc(2000, (20, 15), layout, jclass=10, mclass=10), desc(1000, (20, 15), layout, jclass=20, mclass=15)]
        n, D, S, O = sets(ds)
        yield f"multi_step {name}", lambda a=(n, D, S), O=O: lib.jss_multi_step(*a, ptrs(n), O, 0, STREAM)
        yield f"multi_rollout {name} n_sub=2", lambda a=(n, D, S, O): lib.jss_multi_rollout(*a, FIFO, 7, 0, 2, FORK, 2, STREAMS)

    # ---- step session ----------------------------------------------------------------------------------------------------
    for shape, layout, batch, slots in (("p16", "shared-compact", 512, 0), ("p32", "own-medium", 64, 2), ("w1", "own-full", 64, 0),
                                        ("w2", "shared-full", 8, 1), ("w1", "map-full", 100000, 0)):
        tag = f"{shape}/{layout}/b{batch} slots={slots}"
        d, s, o = desc(batch, shape, layout), state(), out()
        ses = _abi.JssSession(mail=ptr(), progress=ptr(), status=ptr(), depth=4, timeout_ms=0, slots=slots)
        yield f"session_open {tag}", lambda d=d, s=s, o=o, ses=ses: lib.jss_session_open(byref(d), byref(s), byref(o), byref(ses), STREAM)
        yield f"session_post {tag}", lambda d=d, ses=ses: lib.jss_session_post(byref(d), byref(ses), ptr(), 0, 2, 0, STREAM)
        yield f"session_wait {tag}", lambda d=d, ses=ses: lib.jss_session_wait(byref(d), byref(ses), 2, STREAM)
        yield f"session_step {tag}", lambda d=d, ses=ses: lib.jss_session_step(byref(d), byref(ses), ptr(), 2, STREAM)
        yield f"session_close {tag}", lambda d=d, ses=ses: lib.jss_session_close(byref(d), byref(ses), 3, STREAM)
        yield f"session_wait after close {tag}", lambda d=d, ses=ses: lib.jss_session_wait(byref(d), byref(ses), 3, STREAM)

    # ---- instances and clones ----------------------------------------------------------------------------------------------
    for batch, which, seeds in ((1000, False, True), (1000, True, True), (65536, False, False), (0, False, True)):
        d, s = desc(batch, "p32", "own-full"), state()
        g = _abi.JssGen(ops=ptr(), rem=ptr(), inst=ptr(), time_seed=ptr() if seeds else None, machine_seed=ptr() if seeds else None,
                        actions=None, seed=3, jobs=20, machines=15, dur_low=1, dur_high=99)
        yield f"generate b{batch} which={which} seeds={seeds}", lambda d=d, s=s, g=g, w=which: lib.jss_generate(
            byref(d), byref(s), byref(g), ptr() if w else None, STREAM)
    for layout in LAYOUTS:
        for n_dst in (0, 2, 777):
            dd, sd = desc(n_dst, "p32", layout), desc(333, "p32", layout)
            dst = _abi.JssCloneDst(ptr(), ptr(), ptr(), ptr())
            yield f"clone {layout} {n_dst} <- 333", lambda a=(byref(dd), byref(state()), byref(out()), byref(dst), byref(sd), byref(
                state()), byref(out())): lib.jss_clone(*a, ptr(), STREAM)

    # ---- the caller's selectors: weighted rules and key tables ---------------------------------------------------------
    # (the four kernel shapes, the batch's instances in one shared table and in per-env tables, one weight row / key table for
    #  every env and one per env; rollouts of one iteration and of several; lookahead with candidates and with none)
    for shape in SHAPES:
        J, M = SHAPES[shape]
        for layout in ("shared-full", "own-full"):
            for per_env in (False, True):
                tag = f"{shape}/{layout}/b1000 {'per-env' if per_env else 'shared'}"
                d, s, o = desc(1000, shape, layout), state(), out()
                rule = _abi.JssRule(ptr(), _abi.RW_N if per_env else 0)
                keys = _abi.JssKeys(ptr(), J * M if per_env else 0, _abi.KEY_NEVER_NOPE)
                for family, sel in (("rule", rule), ("key", keys)):
                    fn = lambda verb, family=family: getattr(lib, f"jss_{family}_{verb}")      # noqa: E731
                    yield f"{family}_policy {tag}", lambda d=d, s=s, sel=sel, fn=fn: fn("policy")(
                        byref(d), byref(s), byref(sel), 7, 0, ptr(), STREAM)
                    for n_iter in (1, 5):
                        yield f"{family}_rollout n_iter={n_iter} {tag}", lambda d=d, s=s, o=o, sel=sel, fn=fn, n=n_iter: fn("rollout")(
                            byref(d), byref(s), byref(o), byref(sel), 7, 0, n, 0, STREAM)
                    for n in (777, 0):
                        la = _abi.JssLookahead(n=n, parent=ptr(), action=ptr(), id_base=0, makespan=ptr(), steps=ptr(), reward_num=ptr())
                        yield f"{family}_lookahead n={n} {tag}", lambda d=d, s=s, la=la, sel=sel, fn=fn: fn("lookahead")(
                            byref(d), byref(s), byref(la), byref(sel), 7, 0, 0, STREAM)


def main(lib_path, log_path):
    lib = _abi.bind(C.CDLL(lib_path))
    search = _abi.bind_keys(_abi.bind_rules(_abi.bind_search(lib)))
    fd = os.open(log_path, os.O_WRONLY | os.O_APPEND | os.O_CREAT)
    for name, thunk in calls(lib, search):
        os.write(fd, f"# {name}\n".encode())
        rc = thunk()
        os.write(fd, f"-> {rc}\n".encode())
    os.close(fd)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
