"""Which instance a persistent solve call launches (csrc/ipm_plan.h: plan_persist, asked through
noc_debug_ipm_plan) -- host logic, checked here without a GPU for a device of 1024 SIMDs (256 CUs:
MI355X).  The GPU suites show that whatever ran gave the right doubles; this table shows what runs,
so that a policy slip (a batch silently losing its speculative candidates, say) fails a test and
not only a bench line.

Every expected value is worked out by hand from the rules as they stood in ipm_persistent.hip /
ipm_wide.hip before the plan existed (use_wide, spec_auto, heavy_count, solve_t, solve_w,
solve_split, wide_waves), never by calling the plan.  LDS bytes, with
  slots(N) = (N nu (nx + 1) + nx + 1) & ~1,  xu(N) = ((N + 1) nx + N nu + 1) & ~1  doubles:
  one wave:       8 slots + 64 (the parked state) + 16, + 8 xu with x, u in LDS
  SPEC waves:     8 (SPEC (slots + 8 + xu) + 6 SPEC)
  wide, cart-pole: 8 (28 N + 25 + 72 W)   (WideLds: compact A 4, B 2, Q 3, R 1, M 1 per stage)
"""
import ctypes
import os
import subprocess
import sys

import pytest

SIMDS = 1024
RESUME = 2  # NOC_WS_RESUME


@pytest.fixture
def plan(monkeypatch):
    """plan(family, N, B, ordered=False, resume=False, params=False, **env) -> dict of the plan,
    with only the named NOC_PERSIST_* / NOC_WIDE_WAVES variables set."""
    from noc import _lib, problems
    lib = _lib.load()
    fams = {"cartpole": problems.cartpole(0.005).family.to_c(),
            "pendulum": problems.pendulum(0.02).family.to_c(),
            "linear8": problems.double_integrators(4, 0.001).family.to_c()}

    def launch(out, base):
        names = ("wps", "spec", "resume", "xlds", "struct", "grid", "lds")
        return {n: out[base + i] for i, n in enumerate(names)}

    def ask(family, N, B, ordered=False, resume=False, params=False, **env):
        for k in list(os.environ):
            if k.startswith("NOC_PERSIST_") or k == "NOC_WIDE_WAVES":
                monkeypatch.delenv(k)
        for k, v in env.items():
            monkeypatch.setenv("NOC_WIDE_WAVES" if k == "WIDE_WAVES" else "NOC_PERSIST_" + k, str(v))
        out = _lib.ipm_plan(lib, fams[family], N, B, flags=RESUME if resume else 0, ordered=ordered,
                            with_params=params, simds=SIMDS)
        p = {"family": {0: "none", 1: "one-wave", 2: "wide"}[out[_lib.PLAN_FAMILY]],
             "wide_waves": out[_lib.PLAN_WIDE_WAVES], "wide_lds": out[_lib.PLAN_WIDE_LDS],
             "heavy": out[_lib.PLAN_HEAVY], "rest": launch(out, _lib.PLAN_REST)}
        p.update(launch(out, _lib.PLAN_MAIN))
        return p
    return ask


def sub(p, *keys):
    return tuple(p[k] for k in keys)


ONE = ("family", "wps", "spec", "resume", "xlds", "struct", "grid", "lds", "heavy")


def test_unordered_fresh_launch_cartpole_n200(plan):
    # candidates: 4 while 4 B <= #SIMDs, 2 while 2 B <= #SIMDs; one wave per SIMD while B <= #SIMDs.
    # B = 1 is not wide: the candidates win at N <= 320.  SPEC LDS: 8 (SPEC 2016 + 6 SPEC)
    for B, spec, lds in ((1, 4, 64704), (256, 4, 64704), (257, 2, 32352), (512, 2, 32352)):
        assert sub(plan("cartpole", 200, B), *ONE) == ("one-wave", 1, spec, 0, 1, 1, B, lds, 0), B
    for B, wps in ((513, 1), (1024, 1), (1025, 2), (4096, 2)):
        assert sub(plan("cartpole", 200, B), *ONE) == ("one-wave", wps, 1, 0, 1, 1, B, 16144, 0), B


def test_ordered_resume_and_the_heavy_first_split(plan):
    p = plan("cartpole", 200, 1024, ordered=True, resume=True)
    assert sub(p, *ONE) == ("one-wave", 1, 1, 1, 1, 1, 1024, 16144, 0)
    for B in (1025, 2048):  # #SIMDs < B <= 2 #SIMDs, N <= 320: #SIMDs / 8 heavy at two candidates
        p = plan("cartpole", 200, B, ordered=True, resume=True)
        assert sub(p, *ONE) == ("one-wave", 1, 2, 1, 1, 1, 128, 32352, 128), B
        assert p["rest"] == dict(wps=2, spec=1, resume=1, xlds=1, struct=1, grid=B - 128, lds=16144), B
    for N, B, lds in ((200, 2049, 16144), (321, 2048, 12960)):  # N = 321: x, u leave LDS at 2 waves
        p = plan("cartpole", N, B, ordered=True, resume=True)
        assert sub(p, "family", "wps", "spec", "grid", "lds", "heavy") == ("one-wave", 2, 1, B, lds, 0), (N, B)
        assert p["rest"]["grid"] == 0
    p = plan("cartpole", 320, 2048, ordered=True, resume=True)  # the last horizon of the default split
    assert sub(p, "spec", "grid", "lds", "heavy") == (2, 128, 8 * (2 * (1604 + 8 + 1604) + 12), 128)
    assert sub(p["rest"], "wps", "xlds", "lds") == (2, 0, 12912)
    # an order alone (a fresh cost-ordered launch) splits too; without an order nothing does
    assert plan("cartpole", 200, 2048, ordered=True)["heavy"] == 128
    assert plan("cartpole", 200, 2048, resume=True)["heavy"] == 0
    # an ordered launch runs no candidates, whatever the batch
    assert sub(plan("cartpole", 200, 8, ordered=True), "family", "wps", "spec") == ("one-wave", 1, 1)


def test_xlds_boundaries(plan):
    # two waves per SIMD: 20 KB per wave
    assert sub(plan("cartpole", 254, 1025), "wps", "xlds", "lds") == (2, 1, 20464)
    assert sub(plan("cartpole", 255, 1025), "wps", "xlds", "lds") == (2, 0, 10320)  # 20 560 B with x, u
    assert sub(plan("cartpole", 320, 1025), "wps", "xlds", "lds") == (2, 0, 12912)
    # one wave per SIMD: 40 KB
    assert sub(plan("cartpole", 320, 1024), "wps", "spec", "xlds", "lds") == (1, 1, 1, 25744)
    assert sub(plan("cartpole", 510, 1024), "wps", "xlds", "lds") == (1, 1, 40944)
    assert sub(plan("cartpole", 511, 1024), "wps", "xlds", "lds") == (1, 0, 20560)  # 41 040 B with x, u


def test_candidate_lds_boundary(plan):
    # 40 KB per wave: N = 509 gives 40 912 B per wave at four candidates, N = 510 40 976 B -- and
    # then one wave, not two
    assert sub(plan("cartpole", 509, 1, WIDE=0), *ONE) == ("one-wave", 1, 4, 0, 1, 1, 1, 163648, 0)
    assert sub(plan("cartpole", 510, 1, WIDE=0), *ONE) == ("one-wave", 1, 1, 0, 1, 1, 1, 40944, 0)
    assert sub(plan("cartpole", 509, 300, WIDE=0), "spec", "lds") == (2, 81824)
    assert sub(plan("cartpole", 510, 300, WIDE=0), "spec", "lds") == (1, 40944)  # 81 952 B at two


def test_wide_kernel(plan):
    assert sub(plan("cartpole", 400, 1), "family", "wide_waves", "wide_lds") == ("wide", 4, 8 * (11225 + 288))
    assert sub(plan("cartpole", 321, 1), "family", "wide_waves") == ("wide", 4)  # past the candidates
    assert sub(plan("cartpole", 320, 1), "family", "spec") == ("one-wave", 4)
    assert sub(plan("cartpole", 400, 256), "family", "wide_waves") == ("wide", 4)
    assert sub(plan("cartpole", 400, 257), "family", "wps", "spec") == ("one-wave", 1, 2)  # B > #CUs
    assert sub(plan("pendulum", 200, 1), "family", "wide_waves") == ("wide", 4)
    assert sub(plan("pendulum", 129, 1), "family", "wide_waves") == ("wide", 4)
    # N <= 128: the one-wave kernel; pendulum has no one-wave-per-SIMD instance
    assert sub(plan("pendulum", 128, 1), *ONE) == ("one-wave", 2, 1, 0, 1, 1, 1, 8 * (386 + 10 + 386), 0)
    assert sub(plan("pendulum", 200, 257), "family", "wps", "spec", "grid") == ("one-wave", 2, 1, 257)
    # the choice ignores order and resume: a capped B = 1 solve resumes on the family it started on
    assert plan("cartpole", 400, 1, ordered=True, resume=True)["family"] == "wide"
    assert sub(plan("cartpole", 200, 1, resume=True), "family", "spec", "resume") == ("one-wave", 4, 1)
    # forced on beyond one trajectory per CU: two waves where two workgroups fit a CU (80 KB - 512 B)
    assert sub(plan("cartpole", 200, 257, WIDE=1), "family", "wide_waves", "wide_lds") == ("wide", 2, 8 * (5625 + 144))
    assert sub(plan("cartpole", 357, 257, WIDE=1), "family", "wide_waves", "wide_lds") == ("wide", 2, 81320)
    assert sub(plan("cartpole", 358, 257, WIDE=1), "family", "wide_waves") == ("wide", 4)  # 81 544 B at two
    assert sub(plan("cartpole", 200, 256, WIDE=1), "family", "wide_waves") == ("wide", 4)
    assert plan("cartpole", 400, 1, WIDE=0)["family"] == "one-wave"
    assert sub(plan("cartpole", 400, 1, WIDE_WAVES=2), "family", "wide_waves", "wide_lds") == ("wide", 2, 8 * (11225 + 144))
    assert sub(plan("cartpole", 200, 257, WIDE=1, WIDE_WAVES=4), "family", "wide_waves") == ("wide", 4)
    assert sub(plan("cartpole", 400, 1, WIDE_WAVES=3), "family", "wide_waves") == ("wide", 4)  # not 2 | 4


def test_per_trajectory_parameters_never_get_wide_candidates_or_a_split(plan):
    for N in (200, 400):
        assert sub(plan("cartpole", N, 1, params=True), "family", "wps", "spec", "struct", "grid") == \
            ("one-wave", 1, 1, 1, 1), N
    assert sub(plan("cartpole", 200, 1024, params=True), "wps", "spec", "lds") == (1, 1, 16144)
    assert sub(plan("cartpole", 200, 1025, params=True), "wps", "spec", "lds") == (2, 1, 16144)
    p = plan("cartpole", 200, 2048, ordered=True, resume=True, params=True)
    assert sub(p, *ONE) == ("one-wave", 2, 1, 1, 1, 1, 2048, 16144, 0)
    assert plan("pendulum", 200, 1, params=True)["family"] == "one-wave"
    # the twin is the structure-aware instance whatever NOC_PERSIST_STRUCT says; WIDE=1 does not apply
    assert sub(plan("cartpole", 200, 1, params=True, STRUCT=0, WIDE=1), "family", "struct") == ("one-wave", 1)
    assert sub(plan("cartpole", 200, 1025, params=True, XLDS=0), "xlds", "lds") == (0, 8112)


def test_each_knob_once(plan):
    # STRUCT=0: the dense instance, no candidates (so B = 1 at N = 200 is wide), no default split
    assert sub(plan("cartpole", 200, 300, STRUCT=0), *ONE) == ("one-wave", 1, 1, 0, 1, 0, 300, 16144, 0)
    assert plan("cartpole", 200, 1, STRUCT=0)["family"] == "wide"
    p = plan("cartpole", 200, 1025, ordered=True, resume=True, STRUCT=0)
    assert sub(p, "wps", "struct", "grid", "heavy") == (2, 0, 1025, 0)
    # ... and a forced split's heavy half is the dense one-wave-per-SIMD instance
    p = plan("cartpole", 200, 1025, ordered=True, resume=True, STRUCT=0, HEAVY=64, HEAVY_SPEC=2)
    assert sub(p, *ONE) == ("one-wave", 1, 1, 1, 1, 0, 64, 16144, 64)
    assert p["rest"] == dict(wps=2, spec=1, resume=1, xlds=1, struct=0, grid=961, lds=16144)
    # SPEC forces the candidates (not on an ordered launch), within the LDS cap
    assert sub(plan("cartpole", 200, 300, SPEC=1), "family", "wps", "spec") == ("one-wave", 1, 1)
    assert plan("cartpole", 200, 1, SPEC=1)["family"] == "wide"
    assert sub(plan("cartpole", 200, 1, SPEC=2), "family", "spec", "lds") == ("one-wave", 2, 32352)
    assert sub(plan("cartpole", 200, 600, SPEC=4), "family", "wps", "spec", "grid") == ("one-wave", 1, 4, 600)
    assert sub(plan("cartpole", 200, 1025, SPEC=4), "wps", "spec") == (2, 1)  # needs one wave per SIMD
    assert plan("cartpole", 200, 300, SPEC=3)["spec"] == 1
    assert plan("cartpole", 200, 300, ordered=True, SPEC=4)["spec"] == 1
    assert plan("cartpole", 510, 1, SPEC=4, WIDE=0)["spec"] == 1
    assert plan("pendulum", 100, 1, SPEC=4)["spec"] == 1  # the families with a one-wave instance only
    # XLDS=0: x, u stay in the workspace
    assert sub(plan("cartpole", 200, 1025, XLDS=0), "xlds", "lds") == (0, 8112)
    assert sub(plan("cartpole", 200, 1024, XLDS=0), "wps", "xlds", "lds") == (1, 0, 8112)
    # HEAVY_SPEC=0: the default split is off
    assert plan("cartpole", 200, 1025, ordered=True, resume=True, HEAVY_SPEC=0)["heavy"] == 0
    # HEAVY=<n>: its own batch bounds, any horizon; plain one-wave heavy half unless HEAVY_SPEC=2
    assert plan("cartpole", 200, 1024, ordered=True, resume=True, HEAVY=64)["heavy"] == 0
    p = plan("cartpole", 200, 1025, ordered=True, resume=True, HEAVY=64)
    assert sub(p, "wps", "spec", "grid", "heavy") == (1, 1, 64, 64) and sub(p["rest"], "wps", "grid") == (2, 961)
    p = plan("cartpole", 321, 2049, ordered=True, resume=True, HEAVY=64)
    assert sub(p, "wps", "spec", "xlds", "heavy") == (1, 1, 1, 64) and sub(p["rest"], "wps", "xlds", "grid") == (2, 0, 1985)
    assert plan("cartpole", 200, 512, ordered=True, resume=True, HEAVY=64, HEAVY_SPEC=2)["heavy"] == 0
    p = plan("cartpole", 200, 513, ordered=True, resume=True, HEAVY=64, HEAVY_SPEC=2)
    assert sub(p, "wps", "spec", "grid", "heavy") == (1, 2, 64, 64) and sub(p["rest"], "wps", "grid") == (1, 449)
    assert plan("cartpole", 200, 2048, HEAVY=64)["heavy"] == 0  # no order, no split
    p = plan("cartpole", 200, 2048, ordered=True, HEAVY=4096)  # at most #SIMDs / 2
    assert sub(p, "heavy", "grid") == (512, 512) and p["rest"]["grid"] == 1536
    assert plan("cartpole", 200, 2048, ordered=True, HEAVY=-3)["heavy"] == 0
    assert plan("pendulum", 100, 2048, ordered=True, HEAVY=64)["heavy"] == 0  # no one-wave instance


def test_waves_knob_is_read_once_and_turns_the_split_off():
    """NOC_PERSIST_WAVES is the one switch read once per process: asked in a process of its own."""
    code = ("import ctypes\nfrom noc import _lib, problems\nlib = _lib.load()\n"
            "f = problems.cartpole(0.005).family.to_c()\n"
            "for a in ((200, 1, 0, False), (200, 2048, 2, True)):\n"
            "    o = _lib.ipm_plan(lib, f, a[0], a[1], flags=a[2], ordered=a[3], simds=1024)\n"
            "    print(o[_lib.PLAN_FAMILY], o[_lib.PLAN_HEAVY], *o[_lib.PLAN_MAIN:_lib.PLAN_MAIN + 2])\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("NOC_PERSIST_")}
    env["NOC_PERSIST_WAVES"] = "2"
    env["PYTHONPATH"] = os.pathsep.join(sys.path)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True)
    # family, heavy, wps, spec: B = 1 is still not wide (the candidate rule is asked without the
    # register budget) but runs two waves per SIMD, so no candidates; and no split
    assert out.stdout.split("\n")[:2] == ["1 0 2 1", "1 0 2 1"]


def test_unsupported_and_argument_errors(plan):
    from noc import _lib, problems
    lib = _lib.load()
    assert plan("linear8", 100, 4)["family"] == "none"        # nx = 8: the launch-per-phase driver
    assert plan("cartpole", 1635, 4)["family"] == "one-wave"  # 65 520 B of LDS
    assert plan("cartpole", 1636, 4)["family"] == "none"      # 65 552 B
    assert plan("cartpole", 2 ** 31 - 1, 4)["family"] == "none"
    cart = problems.cartpole(0.005).family.to_c()
    out = (ctypes.c_int * _lib.PLAN_INTS)()
    bad = cart.__class__.from_buffer_copy(cart)
    bad.nx = 3
    assert lib.noc_debug_ipm_plan(ctypes.byref(bad), 100, 4, 0, 0, 0, SIMDS, out, _lib.PLAN_INTS) == 0
    assert out[_lib.PLAN_FAMILY] == 0
    assert lib.noc_debug_ipm_plan(None, 100, 4, 0, 0, 0, SIMDS, out, _lib.PLAN_INTS) < 0
    assert lib.noc_debug_ipm_plan(ctypes.byref(cart), 100, 4, 0, 0, 0, SIMDS, None, _lib.PLAN_INTS) < 0
    assert lib.noc_debug_ipm_plan(ctypes.byref(cart), 100, 4, 0, 0, 0, SIMDS, out, _lib.PLAN_INTS - 1) < 0
    assert lib.noc_debug_ipm_plan(ctypes.byref(cart), 0, 4, 0, 0, 0, SIMDS, out, _lib.PLAN_INTS) < 0
    assert lib.noc_debug_ipm_plan(ctypes.byref(cart), 100, -1, 0, 0, 0, SIMDS, out, _lib.PLAN_INTS) < 0
    assert lib.noc_debug_ipm_plan(ctypes.byref(cart), 100, 4, 8, 0, 0, SIMDS, out, _lib.PLAN_INTS) < 0
    assert b"flags" in lib.noc_last_error()


@pytest.mark.parametrize("env", [{}, {"NOC_PERSIST_HEAVY_SPEC": "0"}, {"NOC_PERSIST_SPEC": "1"},
                                 {"NOC_PERSIST_STRUCT": "0"}])
def test_python_heavy_split_rule_moved_not_changed(monkeypatch, env):
    """BatchedIPM._heavy_split_eligible asks the plan; it used to restate the rule.  Its answers
    over the boundary batches, horizons, both families and the environment cases it read are the
    restated rule's (the engine is assembled without a device: the predicate reads these fields)."""
    from noc import _lib, problems
    from noc.ipm import BatchedIPM
    for k in list(os.environ):
        if k.startswith("NOC_PERSIST_") or k == "NOC_WIDE_WAVES":
            monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(BatchedIPM, "_simds", lambda self: SIMDS)
    for ocp in (problems.cartpole(0.005), problems.pendulum(0.02)):
        for N in (320, 321):
            for B in (1024, 1025, 2048, 2049):
                for persistent in (True, False):
                    e = object.__new__(BatchedIPM)
                    e.family, e.fam_c, e.N, e.Bt = ocp.family, ocp.family.to_c(), N, B
                    e.persistent, e._lib, e.ws = persistent, _lib.load(), _lib.NocIpmWs()
                    was = (not env and persistent and ocp.family.kind == _lib.FAMILY_CARTPOLE
                           and N <= 320 and SIMDS < B <= 2 * SIMDS)
                    assert e._heavy_split_eligible() == was, (ocp.family.kind, N, B, persistent, env)
