"""Argument errors of the C ABI are the same in both libraries: every entry point of libjss_hip.so and of its host-core twin
libjss_cpu.so starts with the same check (jssenv_amd/csrc/jss_abi_checks.hpp).  A table of malformed argument lists, one
or more rows per entry point, runs against the twin, the emulator library (tests/emu: the HIP library's host code compiled
unchanged) and -- only where no GPU is visible, so that a row let through by mistake cannot launch on host pointers --
the real libjss_hip.so.  Every library must return the code the table gives, and no buffer the call could write may
change: an argument error touches nothing, in multi-set calls neither."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from jssenv_amd import _abi
from jssenv_amd._abi import E_KIND, E_NULL, E_SESSION, E_SHAPE

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu"))

B, J, M = 2, 4, 3              # every set: 2 envs, 4 jobs, 3 machines
NF, NFC, NFM = _abi.NF, _abi.NFC, _abi.NFM
KIND_BAD = 99
MWR, CR = _abi.POLICY["MWR"], _abi.POLICY["CR"]
CR_F64 = _abi.POLICY_CR_F64


class World:
    """Host buffers for one call: every pointer an argument carries is a 64 KiB buffer of random bytes of its own, so that
    a write anywhere shows up as a changed byte."""

    def __init__(self, lib):
        self.lib = lib
        self.bufs = []
        self.rng = np.random.default_rng(1)
        self.streams = (C.c_void_p * 16)()

    def p(self):
        b = self.rng.integers(0, 256, size=1 << 16, dtype=np.uint8)
        self.bufs.append(b)
        return b.ctypes.data

    def d(self, n_tables=1, **kw):
        d = _abi.JssDesc(batch=B, jmax=J, mmax=M, n_tables=n_tables, ops=self.p(), rem=self.p(), inst=self.p())
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def s(self, **kw):
        s = _abi.JssState(*(self.p() for _ in range(6)))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def o(self, **kw):
        o = _abi.JssOut(*(self.p() for _ in range(5)))
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    def traj(self):
        return _abi.JssTraj(self.p(), self.p(), self.p(), self.p(), self.p(), 0)

    def sess(self, **kw):
        s = _abi.JssSession(mail=self.p(), progress=self.p(), status=self.p(), depth=4, timeout_ms=0, slots=0)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    def lg(self, **kw):
        lg = _abi.JssLogits(logits=self.p(), row=0, dtype=_abi.LOGITS_F32, temperature=1.0, action=self.p(),
                            logp=self.p(), entropy=self.p())
        for k, v in kw.items():
            setattr(lg, k, v)
        return lg

    def gen(self, **kw):
        g = _abi.JssGen(ops=self.p(), rem=self.p(), inst=self.p(), time_seed=self.p(), machine_seed=self.p(), actions=None,
                        seed=0, jobs=J, machines=M, dur_low=1, dur_high=99)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def dst(self, **kw):
        t = _abi.JssCloneDst(self.p(), self.p(), self.p(), self.p())
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    @staticmethod
    def arr(typ, items):
        """A pointer array of a multi-set call: None entries are NULL."""
        P = C.POINTER(typ)
        return (P * len(items))(*[P() if x is None else C.pointer(x) for x in items])

    def ptrs(self, items):
        return (C.c_void_p * len(items))(*items)

    def sets(self, n=2, bad=None, **over):
        """n sets' (descs, states, outs) arrays; bad = (set index, 'd' | 's' | 'o', overrides) spoils one set."""
        ds, ss, os_ = [], [], []
        for i in range(n):
            kw = {"d": {}, "s": {}, "o": {}}
            if bad and bad[0] == i:
                kw[bad[1]] = bad[2]
            ds.append(None if kw["d"] is None else self.d(**{**over, **kw["d"]}))
            ss.append(self.s(**kw["s"]))
            os_.append(self.o(**kw["o"]))
        return self.arr(_abi.JssDesc, ds), self.arr(_abi.JssState, ss), self.arr(_abi.JssOut, os_)


def _rows():
    R = []

    def row(name, entry, expected, build):
        R.append(pytest.param(entry, build, expected, id=name))

    # ---- one env set: JssDesc / JssState / JssOut (check_args), through jss_reset ------------------------------------
    row("reset-desc-null", "jss_reset", E_NULL, lambda w: (None, w.s(), w.o(), None, None))
    row("reset-state-null", "jss_reset", E_NULL, lambda w: (w.d(), None, w.o(), None, None))
    row("reset-out-null", "jss_reset", E_NULL, lambda w: (w.d(), w.s(), None, None, None))
    row("reset-all-null", "jss_reset", E_NULL, lambda w: (None, None, None, None, None))
    for f in ("ops", "inst"):
        row(f"reset-desc-{f}-null", "jss_reset", E_NULL, lambda w, f=f: (w.d(**{f: None}), w.s(), w.o(), None, None))
    for f in ("env", "env_const", "job", "solution", "machine"):
        row(f"reset-state-{f}-null", "jss_reset", E_NULL, lambda w, f=f: (w.d(), w.s(**{f: None}), w.o(), None, None))
    for f in ("real_obs", "action_mask", "reward", "done", "makespan"):
        row(f"reset-out-{f}-null", "jss_reset", E_NULL, lambda w, f=f: (w.d(), w.s(), w.o(**{f: None}), None, None))
    for name, kw in (("batch-neg", {"batch": -1}), ("jmax-0", {"jmax": 0}), ("jmax-129", {"jmax": 129}),
                     ("mmax-1", {"mmax": 1}), ("mmax-65", {"mmax": 65}), ("ntables-0", {"n_tables": 0}),
                     ("ntables-3", {"n_tables": 3}), ("records-5", {"record_ints": 5}),
                     ("compact-per-env", {"record_ints": NFC, "n_tables": 2}),
                     ("medium-shared", {"record_ints": NFM, "n_tables": 1}),
                     ("medium-mmax-33", {"record_ints": NFM, "n_tables": 2, "mmax": 33})):
        row(f"reset-{name}", "jss_reset", E_SHAPE, lambda w, kw=kw: (w.d(**kw), w.s(), w.o(), None, None))
    row("reset-kernel-8", "jss_reset", E_KIND, lambda w: (w.d(kernel=8), w.s(), w.o(), None, None))
    row("reset-null-before-shape", "jss_reset", E_NULL, lambda w: (w.d(jmax=0), w.s(env=None), w.o(), None, None))
    row("reset-kind-before-records", "jss_reset", E_KIND, lambda w: (w.d(kernel=8, record_ints=5), w.s(), w.o(), None, None))
    row("advance-desc-null", "jss_advance", E_NULL, lambda w: (None, w.s(), None, None, w.o(), None))
    row("advance-out-null", "jss_advance", E_NULL, lambda w: (w.d(), w.s(), None, None, None, None))
    row("advance-jmax-0", "jss_advance", E_SHAPE, lambda w: (w.d(jmax=0), w.s(), None, None, w.o(), None))

    # ---- step, step_autoreset, step_logits ----------------------------------------------------------------------------
    for entry in ("jss_step", "jss_step_autoreset"):
        row(f"{entry}-actions-null", entry, E_NULL, lambda w: (w.d(), w.s(), None, w.o(), None))
        row(f"{entry}-out-null", entry, E_NULL, lambda w: (w.d(), w.s(), w.p(), None, None))
        row(f"{entry}-desc-before-actions", entry, E_KIND, lambda w: (w.d(kernel=8), w.s(), None, w.o(), None))
    L = "jss_step_logits"
    row("logits-lg-null", L, E_NULL, lambda w: (w.d(), w.s(), None, 0, 0, w.o(), None))
    row("logits-logits-null", L, E_NULL, lambda w: (w.d(), w.s(), w.lg(logits=None), 0, 0, w.o(), None))
    row("logits-action-null", L, E_NULL, lambda w: (w.d(), w.s(), w.lg(action=None), 0, 0, w.o(), None))
    row("logits-row-short", L, E_SHAPE, lambda w: (w.d(), w.s(), w.lg(row=J), 0, 0, w.o(), None))
    row("logits-row-negative", L, E_SHAPE, lambda w: (w.d(), w.s(), w.lg(row=-1), 0, 0, w.o(), None))
    row("logits-row-huge", L, E_SHAPE, lambda w: (w.d(), w.s(), w.lg(row=(1 << 24) + 1), 0, 0, w.o(), None))
    row("logits-dtype", L, E_KIND, lambda w: (w.d(), w.s(), w.lg(dtype=2), 0, 0, w.o(), None))
    row("logits-temperature-neg", L, E_KIND, lambda w: (w.d(), w.s(), w.lg(temperature=-1.0), 0, 0, w.o(), None))
    row("logits-temperature-nan", L, E_KIND, lambda w: (w.d(), w.s(), w.lg(temperature=float("nan")), 0, 0, w.o(), None))
    row("logits-desc-before-lg", L, E_SHAPE, lambda w: (w.d(jmax=0), w.s(), None, 0, 0, w.o(), None))
    row("logits-out-null", L, E_NULL, lambda w: (w.d(), w.s(), w.lg(), 0, 0, None, None))

    # ---- policy (kind checks: check_kind) -----------------------------------------------------------------------------
    P = "jss_policy"
    row("policy-all-null", P, E_NULL, lambda w: (None, None, 0, 0, 0, None, None))
    row("policy-actions-null", P, E_NULL, lambda w: (w.d(), w.s(), 0, 0, 0, None, None))
    row("policy-actions-before-kind", P, E_NULL, lambda w: (w.d(), w.s(), KIND_BAD, 0, 0, None, None))
    row("policy-desc-before-actions", P, E_SHAPE, lambda w: (w.d(mmax=1), w.s(), 0, 0, 0, None, None))
    for name, kind, kw, code in (("kind-99", KIND_BAD, {}, E_KIND), ("kind-neg", -1, {}, E_KIND),
                                 ("kind-bit25", 1 << 25, {}, E_KIND), ("f64-factor-0", CR_F64, {"cr_factor": 0.0}, E_KIND),
                                 ("f64-factor-huge", CR_F64, {"cr_factor": 1e301}, E_KIND),
                                 ("f64-with-pq", CR_F64 | (3 << 8) | (2 << 16), {"cr_factor": 1.5}, E_KIND),
                                 ("f64-on-spt", 2 | (1 << 24), {"cr_factor": 1.5}, E_KIND),
                                 ("pq-on-spt", 2 | (3 << 8) | (2 << 16), {}, E_KIND),
                                 ("pq-q3", CR | (3 << 8) | (3 << 16), {}, E_KIND),
                                 ("pq-q128", CR | (3 << 8) | (128 << 16), {}, E_KIND),
                                 ("pq-p0", CR | (2 << 16), {}, E_KIND),
                                 ("mwr-rem-null", MWR, {"rem": None}, E_NULL),
                                 ("cr-rem-null", CR, {"rem": None}, E_NULL)):
        row(f"policy-{name}", P, code, lambda w, kind=kind, kw=kw: (w.d(**kw), w.s(), kind, 0, 0, w.p(), None))

    # ---- rollout, trajectory, steps ----------------------------------------------------------------------------------
    RO = "jss_rollout"
    row("rollout-desc-null", RO, E_NULL, lambda w: (None, w.s(), w.o(), 0, 0, 0, 1, 0, None))
    row("rollout-out-null", RO, E_NULL, lambda w: (w.d(), w.s(), None, 0, 0, 0, 1, 0, None))
    row("rollout-kind", RO, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, 1, 0, None))
    row("rollout-f64", RO, E_KIND, lambda w: (w.d(cr_factor=1.5), w.s(), w.o(), CR_F64, 0, 0, 1, 0, None))
    row("rollout-n-iter", RO, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, -1, 0, None))
    row("rollout-kind-before-n-iter", RO, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, -1, 0, None))
    T = "jss_trajectory"
    row("traj-traj-null", T, E_NULL, lambda w: (w.d(), w.s(), w.o(), None, 0, 0, 0, 1, 0, None))
    row("traj-traj-before-kind", T, E_NULL, lambda w: (w.d(), w.s(), w.o(), None, KIND_BAD, 0, 0, 1, 0, None))
    row("traj-kind", T, E_KIND, lambda w: (w.d(), w.s(), w.o(), w.traj(), KIND_BAD, 0, 0, 1, 0, None))
    row("traj-n-steps", T, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), w.traj(), 0, 0, 0, -1, 0, None))
    row("traj-out-null", T, E_NULL, lambda w: (w.d(), w.s(), None, w.traj(), 0, 0, 0, 1, 0, None))
    S = "jss_steps"
    row("steps-desc-null", S, E_NULL, lambda w: (None, w.s(), w.o(), None, w.p(), 1, None))
    row("steps-desc-null-0-steps", S, E_NULL, lambda w: (None, w.s(), w.o(), None, None, 0, None))
    row("steps-n-steps", S, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), None, w.p(), -1, None))
    row("steps-n-steps-before-actions", S, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), None, None, -1, None))
    row("steps-actions-null", S, E_NULL, lambda w: (w.d(), w.s(), w.o(), w.traj(), None, 1, None))
    row("steps-0-steps-actions-null", S, 0, lambda w: (w.d(), w.s(), w.o(), w.traj(), None, 0, None))

    # ---- step session: the argument part ------------------------------------------------------------------------------
    O = "jss_session_open"
    row("open-desc-null", O, E_NULL, lambda w: (None, w.s(), w.o(), w.sess(), None))
    row("open-session-null", O, E_NULL, lambda w: (w.d(), w.s(), w.o(), None, None))
    for f in ("mail", "progress", "status"):
        row(f"open-{f}-null", O, E_NULL, lambda w, f=f: (w.d(), w.s(), w.o(), w.sess(**{f: None}), None))
    row("open-depth-0", O, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), w.sess(depth=0), None))
    row("open-timeout-neg", O, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), w.sess(timeout_ms=-1), None))
    row("open-batch-0", O, E_SHAPE, lambda w: (w.d(batch=0), w.s(), w.o(), w.sess(), None))
    row("open-slots-3", O, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), w.sess(slots=3), None))
    row("open-desc-before-session", O, E_KIND, lambda w: (w.d(kernel=8), w.s(), w.o(), None, None))
    PO = "jss_session_post"
    row("post-desc-null", PO, E_NULL, lambda w: (None, w.sess(), w.p(), 0, 1, 0, None))
    row("post-session-null", PO, E_NULL, lambda w: (w.d(), None, w.p(), 0, 1, 0, None))
    row("post-mail-null", PO, E_NULL, lambda w: (w.d(), w.sess(mail=None), w.p(), 0, 1, 0, None))
    row("post-actions-null", PO, E_NULL, lambda w: (w.d(), w.sess(), None, 0, 1, 0, None))
    for name, a in (("first-neg", (-1, 1, 0)), ("n-0", (0, 0, 0)), ("waited-neg", (0, 1, -1)),
                    ("waited-ahead", (1, 1, 2)), ("overrun", (0, 5, 0))):
        row(f"post-{name}", PO, E_SESSION, lambda w, a=a: (w.d(), w.sess(), w.p(), *a, None))
    WA = "jss_session_wait"
    row("wait-desc-null", WA, E_NULL, lambda w: (None, w.sess(), 0, None))
    row("wait-progress-null", WA, E_NULL, lambda w: (w.d(), w.sess(progress=None), 0, None))
    row("wait-status-null", WA, E_NULL, lambda w: (w.d(), w.sess(status=None), 0, None))
    row("wait-steps-neg", WA, E_SESSION, lambda w: (w.d(), w.sess(), -1, None))
    ST = "jss_session_step"
    row("step-desc-null", ST, E_NULL, lambda w: (None, w.sess(), w.p(), 0, None))
    for f in ("mail", "progress", "status"):
        row(f"sstep-{f}-null", ST, E_NULL, lambda w, f=f: (w.d(), w.sess(**{f: None}), w.p(), 0, None))
    row("sstep-actions-null", ST, E_NULL, lambda w: (w.d(), w.sess(), None, 0, None))
    row("sstep-step-neg", ST, E_SESSION, lambda w: (w.d(), w.sess(), w.p(), -1, None))
    CL = "jss_session_close"
    row("close-desc-null", CL, E_NULL, lambda w: (None, w.sess(), 0, None))
    row("close-mail-null", CL, E_NULL, lambda w: (w.d(), w.sess(mail=None), 0, None))
    row("close-step-neg", CL, E_SESSION, lambda w: (w.d(), w.sess(), -1, None))

    # ---- rollout_steps, policy_step_steps -------------------------------------------------------------------------------
    RS = "jss_rollout_steps"
    row("rsteps-desc-null", RS, E_NULL, lambda w: (None, w.s(), w.o(), 0, 0, 0, 1, 0, 1, w.streams))
    row("rsteps-out-null-bad-n", RS, E_NULL, lambda w: (w.d(), w.s(), None, 0, 0, 0, -1, 0, 1, w.streams))
    row("rsteps-desc-null-0-steps", RS, E_NULL, lambda w: (None, None, None, 0, 0, 0, 0, 0, 1, None))
    row("rsteps-kind", RS, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, 1, 0, 1, w.streams))
    row("rsteps-kind-before-streams", RS, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, 1, 0, 1, None))
    row("rsteps-kind-0-steps", RS, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, 0, 0, 1, w.streams))
    row("rsteps-n-steps", RS, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, -1, 0, 1, w.streams))
    row("rsteps-n-sub-0", RS, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, 1, 0, 0, w.streams))
    row("rsteps-n-sub-17", RS, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, 1, 0, 17, w.streams))
    row("rsteps-streams-null", RS, E_NULL, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, 1, 0, 1, None))
    row("rsteps-0-steps", RS, 0, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, 0, 0, 1, w.streams))
    PS = "jss_policy_step_steps"
    row("pss-all-null-0-steps", PS, E_NULL, lambda w: (None, None, None, 0, 0, 0, None, 0, 0, 1, None))
    row("pss-null-0-steps", PS, E_NULL, lambda w: (None, None, None, 0, 0, 0, w.p(), 0, 0, 1, w.streams))
    row("pss-out-null", PS, E_NULL, lambda w: (w.d(), w.s(), None, 0, 0, 0, w.p(), 1, 0, 1, w.streams))
    row("pss-out-null-bad-n", PS, E_NULL, lambda w: (w.d(), w.s(), None, 0, 0, 0, w.p(), -1, 0, 1, w.streams))
    row("pss-kind", PS, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, w.p(), 1, 0, 1, w.streams))
    row("pss-kind-before-actions", PS, E_KIND, lambda w: (w.d(), w.s(), w.o(), KIND_BAD, 0, 0, None, 1, 0, 1, None))
    row("pss-mwr-rem-null", PS, E_NULL, lambda w: (w.d(rem=None), w.s(), w.o(), MWR, 0, 0, w.p(), 1, 0, 1, w.streams))
    row("pss-n-steps", PS, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, w.p(), -1, 0, 1, w.streams))
    row("pss-n-sub", PS, E_SHAPE, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, w.p(), 1, 0, 0, w.streams))
    row("pss-actions-null", PS, E_NULL, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, None, 1, 0, 1, w.streams))
    row("pss-streams-null", PS, E_NULL, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, w.p(), 1, 0, 1, None))
    row("pss-actions-null-0-steps", PS, E_NULL, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, None, 0, 0, 1, w.streams))
    row("pss-0-steps", PS, 0, lambda w: (w.d(), w.s(), w.o(), 0, 0, 0, w.p(), 0, 0, 1, w.streams))

    # ---- several env sets: every set checked before any is touched ------------------------------------------------------
    bad_desc = (1, "d", None)                        # set 1's desc NULL
    bad_jmax = (1, "d", {"jmax": 0})
    bad_out = (1, "o", {"done": None})
    MR = "jss_multi_reset"
    row("mreset-descs-null", MR, E_NULL, lambda w: (2, None, w.sets()[1], w.sets()[2], None, None))
    row("mreset-outs-null", MR, E_NULL, lambda w: (2, *w.sets()[:2], None, None, None))
    row("mreset-n-sets-0", MR, E_SHAPE, lambda w: (0, *w.sets(), None, None))
    row("mreset-n-sets-17", MR, E_SHAPE, lambda w: (17, *w.sets(17), None, None))
    row("mreset-later-set-null", MR, E_NULL, lambda w: (2, *w.sets(bad=bad_desc), None, None))
    row("mreset-later-set-shape", MR, E_SHAPE, lambda w: (2, *w.sets(bad=bad_jmax), None, None))
    row("mreset-later-set-out", MR, E_NULL, lambda w: (2, *w.sets(bad=bad_out), None, None))
    MS = "jss_multi_step"

    def mstep(w, n=2, bad=None, actions=True, null_action=None):
        d, s, o = w.sets(n, bad=bad)
        acts = w.ptrs([None if i == null_action else w.p() for i in range(n)]) if actions else None
        return (n, d, s, acts, o, 0, None)
    row("mstep-n-sets-0-actions-null", MS, E_SHAPE, lambda w: mstep(w, n=0, actions=False))
    row("mstep-actions-null", MS, E_NULL, lambda w: mstep(w, actions=False))
    row("mstep-later-action-null", MS, E_NULL, lambda w: mstep(w, null_action=1))
    row("mstep-later-set-shape", MS, E_SHAPE, lambda w: mstep(w, bad=bad_jmax))
    row("mstep-later-set-shape-actions-null", MS, E_SHAPE, lambda w: mstep(w, bad=bad_jmax, actions=False))
    row("mstep-later-set-out", MS, E_NULL, lambda w: mstep(w, bad=bad_out))
    ML = "jss_multi_step_logits"

    def mlogits(w, n=2, bad=None, lgs=None, null_lgs=False):
        d, s, o = w.sets(n, bad=bad)
        lg = None if null_lgs else w.arr(_abi.JssLogits, [w.lg(**(lgs or {}).get(i, {})) if (lgs or {}).get(i, {}) is not None
                                                          else None for i in range(n)])
        return (n, d, s, lg, 0, 0, o, None)
    row("mlogits-lgs-null", ML, E_NULL, lambda w: mlogits(w, null_lgs=True))
    row("mlogits-lgs-null-bad-set", ML, E_NULL, lambda w: mlogits(w, bad=bad_jmax, null_lgs=True))
    row("mlogits-later-lg-null", ML, E_NULL, lambda w: mlogits(w, lgs={1: None}))
    row("mlogits-later-dtype", ML, E_KIND, lambda w: mlogits(w, lgs={1: {"dtype": 7}}))
    row("mlogits-later-row", ML, E_SHAPE, lambda w: mlogits(w, lgs={1: {"row": 2}}))
    row("mlogits-descs-before-logits", ML, E_KIND, lambda w: mlogits(w, bad=(1, "d", {"kernel": 8}), lgs={0: {"row": 2}}))
    row("mlogits-later-set-shape", ML, E_SHAPE, lambda w: mlogits(w, bad=bad_jmax))
    row("mlogits-n-sets-0", ML, E_SHAPE, lambda w: mlogits(w, n=0))
    MP = "jss_multi_policy"

    def mpolicy(w, kind=0, n=2, bad=None, actions=True, null_action=None, **over):
        d, s, _ = w.sets(n, bad=bad, **over)
        acts = w.ptrs([None if i == null_action else w.p() for i in range(n)]) if actions else None
        return (n, d, s, kind, 0, 0, acts, None)
    row("mpolicy-actions-null", MP, E_NULL, lambda w: mpolicy(w, actions=False))
    row("mpolicy-later-action-null", MP, E_NULL, lambda w: mpolicy(w, null_action=1))
    row("mpolicy-kind", MP, E_KIND, lambda w: mpolicy(w, kind=KIND_BAD))
    row("mpolicy-kind-before-action", MP, E_KIND, lambda w: mpolicy(w, kind=KIND_BAD, null_action=1))
    row("mpolicy-later-kind", MP, E_KIND, lambda w: mpolicy(w, kind=CR_F64, cr_factor=1.5, bad=(1, "d", {"cr_factor": -1.0})))
    row("mpolicy-descs-before-kind", MP, E_SHAPE, lambda w: mpolicy(w, kind=CR_F64, cr_factor=-1.0, bad=bad_jmax))
    row("mpolicy-later-set-null", MP, E_NULL, lambda w: mpolicy(w, bad=(1, "s", {"job": None})))
    row("mpolicy-n-sets-17", MP, E_SHAPE, lambda w: mpolicy(w, n=17))
    MO = "jss_multi_rollout"

    def mroll(w, kind=0, n=2, bad=None, n_steps=1, n_sub=1, streams=True):
        d, s, o = w.sets(n, bad=bad)
        return (n, d, s, o, kind, 0, 0, n_steps, 0, n_sub, w.streams if streams else None)
    row("mroll-streams-null", MO, E_NULL, lambda w: mroll(w, streams=False))
    row("mroll-kind", MO, E_KIND, lambda w: mroll(w, kind=KIND_BAD))
    row("mroll-n-steps", MO, E_SHAPE, lambda w: mroll(w, n_steps=-1))
    row("mroll-n-sub-0", MO, E_SHAPE, lambda w: mroll(w, n_sub=0))
    row("mroll-n-sub-17", MO, E_SHAPE, lambda w: mroll(w, n_sub=17))
    row("mroll-n-sub-before-kind", MO, E_SHAPE, lambda w: mroll(w, kind=KIND_BAD, n_sub=0))
    row("mroll-later-set-shape", MO, E_SHAPE, lambda w: mroll(w, bad=bad_jmax))
    row("mroll-later-set-before-n-sub", MO, E_KIND, lambda w: mroll(w, bad=(1, "d", {"kernel": 8}), n_sub=0))
    row("mroll-later-set-0-steps", MO, E_NULL, lambda w: mroll(w, bad=bad_out, n_steps=0))
    row("mroll-0-steps", MO, 0, lambda w: mroll(w, n_steps=0))
    RM = "jss_rollout_steps_multi"

    def rsm(w, kind=0, n=2, bad=None, n_steps=1, streams=True):
        d, s, o = w.sets(n, bad=bad)
        return (n, d, s, o, kind, 0, 0, n_steps, 0, w.streams if streams else None)
    row("rsm-descs-null", RM, E_NULL, lambda w: (2, None, *w.sets()[1:], 0, 0, 0, 1, 0, w.streams))
    row("rsm-streams-null", RM, E_NULL, lambda w: rsm(w, streams=False))
    row("rsm-n-sets-0", RM, E_SHAPE, lambda w: rsm(w, n=0))
    row("rsm-n-steps", RM, E_SHAPE, lambda w: rsm(w, n_steps=-1))
    row("rsm-kind", RM, E_KIND, lambda w: rsm(w, kind=KIND_BAD))
    row("rsm-later-set-shape", RM, E_SHAPE, lambda w: rsm(w, bad=bad_jmax))
    row("rsm-later-set-null", RM, E_NULL, lambda w: rsm(w, bad=bad_desc))
    row("rsm-later-set-rem-null", RM, E_NULL, lambda w: rsm(w, kind=MWR, bad=(1, "d", {"rem": None})))
    row("rsm-later-set-0-steps", RM, E_SHAPE, lambda w: rsm(w, bad=bad_jmax, n_steps=0))
    row("rsm-0-steps", RM, 0, lambda w: rsm(w, n_steps=0))

    # ---- generate ------------------------------------------------------------------------------------------------------
    G = "jss_generate"

    def gen(w, d=None, state=True, **kw):
        return (w.d(**{"n_tables": B, **(d or {})}), w.s() if state else None, w.gen(**kw), None, None)
    row("gen-desc-null", G, E_NULL, lambda w: (None, w.s(), w.gen(), None, None))
    row("gen-gen-null", G, E_NULL, lambda w: (w.d(n_tables=B), w.s(), None, None, None))
    for f in ("ops", "rem", "inst", "time_seed"):
        row(f"gen-{f}-null", G, E_NULL, lambda w, f=f: gen(w, **{f: None}))
    row("gen-table-of-env", G, E_SHAPE, lambda w: gen(w, d={"table_of_env": w.p()}))
    row("gen-derived-state-null", G, E_NULL, lambda w: gen(w, state=False, time_seed=None, machine_seed=None))
    row("gen-derived-env-null", G, E_NULL, lambda w: (w.d(n_tables=B), w.s(env=None), w.gen(time_seed=None, machine_seed=None),
                                                      None, None))
    for name, d, kw in (("batch-neg", {"batch": -1, "n_tables": -1}, {}), ("jmax-0", {"jmax": 0}, {}),
                        ("mmax-0", {"mmax": 0}, {}), ("mmax-65", {"mmax": 65}, {}), ("shared-table", {"n_tables": 1}, {}),
                        ("jobs-0", {}, {"jobs": 0}), ("jobs-big", {}, {"jobs": J + 1}),
                        ("machines-big", {}, {"machines": M + 1}), ("dur-low-0", {}, {"dur_low": 0}),
                        ("dur-inverted", {}, {"dur_low": 9, "dur_high": 8}), ("dur-high-big", {}, {"dur_high": 65536})):
        row(f"gen-{name}", G, E_SHAPE, lambda w, d=d, kw=kw: gen(w, d=d, **kw))

    # ---- clone ---------------------------------------------------------------------------------------------------------
    CO = "jss_clone"

    def clone(w, dd=None, sd=None, dst=True, src_of_dst=True, dsta=None, ssta=None, dout=None):
        return (w.d(**(dd or {})), w.s(**(dsta or {})), w.o(**(dout or {})), w.dst(**dst) if isinstance(dst, dict) else
                (w.dst() if dst else None), w.d(**(sd or {})), w.s(**(ssta or {})), w.o(), w.p() if src_of_dst else None, None)
    row("clone-index-null", CO, E_NULL, lambda w: clone(w, src_of_dst=False))
    row("clone-index-null-before-desc", CO, E_NULL, lambda w: clone(w, dd={"jmax": 0}, src_of_dst=False))
    row("clone-dst-state-null", CO, E_NULL, lambda w: clone(w, dsta={"env": None}))
    row("clone-dst-out-null", CO, E_NULL, lambda w: clone(w, dout={"reward": None}))
    row("clone-src-shape", CO, E_SHAPE, lambda w: clone(w, sd={"mmax": 99}))
    row("clone-dst-before-src", CO, E_KIND, lambda w: clone(w, dd={"kernel": 8}, sd={"jmax": 0}))
    row("clone-jmax-differ", CO, E_SHAPE, lambda w: clone(w, sd={"jmax": J + 1}))
    row("clone-records-differ", CO, E_SHAPE, lambda w: clone(w, dd={"record_ints": NFC}))
    row("clone-shared-vs-own", CO, E_SHAPE, lambda w: clone(w, sd={"n_tables": B}))
    row("clone-map-vs-shared", CO, E_SHAPE, lambda w: clone(w, dd={"table_of_env": w.p(), "n_tables": 3}))
    row("clone-map-n-tables-differ", CO, E_SHAPE, lambda w: clone(w, dd={"table_of_env": w.p(), "n_tables": 3},
                                                                 sd={"table_of_env": w.p(), "n_tables": 5}))
    row("clone-map-dst-null", CO, E_SHAPE, lambda w: clone(w, dd={"table_of_env": w.p(), "n_tables": 3},
                                                          sd={"table_of_env": w.p(), "n_tables": 3}, dst=False))
    row("clone-map-dst-map-null", CO, E_SHAPE, lambda w: clone(w, dd={"table_of_env": w.p(), "n_tables": 3},
                                                              sd={"table_of_env": w.p(), "n_tables": 3}, dst={"table_of_env": None}))
    row("clone-own-dst-null", CO, E_SHAPE, lambda w: clone(w, dd={"n_tables": B}, sd={"n_tables": B}, dst=False))
    row("clone-own-dst-ops-null", CO, E_SHAPE, lambda w: clone(w, dd={"n_tables": B}, sd={"n_tables": B}, dst={"ops": None}))
    row("clone-own-src-rem-null", CO, E_NULL, lambda w: clone(w, dd={"n_tables": B}, sd={"n_tables": B, "rem": None}))
    return R


ROWS = _rows()


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="module")
def libs():
    from emu_backend import build as build_emu
    from jssenv_amd.build import build_cpu_twin, build_extension
    out = {"twin": _abi.bind(C.CDLL(build_cpu_twin())), "emu": _abi.bind(C.CDLL(build_emu()))}
    if not _has_gpu():              # no device: a row let through by mistake fails at its launch instead of reading host pointers
        out["hip"] = _abi.bind(C.CDLL(build_extension()))
    return out


@pytest.mark.parametrize("entry, build, expected", ROWS)
def test_argument_error(libs, entry, build, expected):
    codes = {}
    for name, lib in libs.items():
        w = World(lib)
        args = build(w)
        before = [b.copy() for b in w.bufs]
        codes[name] = getattr(lib, entry)(*args)
        changed = [i for i, (a, b) in enumerate(zip(before, w.bufs)) if not np.array_equal(a, b)]
        assert not changed, f"{name}: {entry} wrote into buffers {changed}"
    assert set(codes.values()) == {expected}, codes


def test_every_entry_point_has_rows():
    covered = {p.values[0] for p in ROWS}
    calls = set(_abi.SYMBOLS) - {"jss_abi_version", "jss_error_string", "jss_backend", "jss_sync_check"}
    assert covered == calls, calls ^ covered


def test_error_strings_agree(libs):
    for code in (0, E_NULL, E_SHAPE, E_KIND, _abi.E_LDS, _abi.E_RESIDENT, E_SESSION):
        texts = {name: lib.jss_error_string(code) for name, lib in libs.items()}
        assert len(set(texts.values())) == 1 and texts["twin"], texts
    assert libs["twin"].jss_error_string(-99) == libs["emu"].jss_error_string(-99) == b"unknown error"
