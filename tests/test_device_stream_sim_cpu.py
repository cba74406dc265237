"""The device entries that share one of the context's two scratch buffers (dev_tmp: the deblocked planes between the two launches of
deblocking + SAO; dev_sao: 4:2:2 SAO parameters and border bytes rewritten for square CTBs) while the caller brings the streams, without
a GPU (tests/device_stream_sim: the three real host sources linked against the model of the HIP runtime of tests/host_frame_sim, which
defers every operation, runs it inside a later HIP call chosen by an eager, a lazy or a seeded random scheduler, and lets a kernel
operation write what its operands hold when it RUNS).  Sessions made from a seed -- one context, 1 to 3 caller streams and sometimes
NULL, 2 to 8 calls with buffers of their own -- must leave every dst as computed from the operands the call was given, with no
violation in the model, also around the k-th launch, hipEventRecord, hipStreamWaitEvent or hipMalloc failing, and without a blocking
HIP call in a call that allocates nothing.  Product and diagnostic build of the host sources, and both under AddressSanitizer + UBSan
and under ThreadSanitizer; all stand-alone programs."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "device_stream_sim")
CSRC = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
SEED = "20261"
SESSIONS = 3000
SANITIZED_SESSIONS = 300
SCHEDULERS = {"eager", "lazy", "random"}
FAULTS = {"launch", "hipEventRecord", "hipStreamWaitEvent", "hipMalloc"}
# mixed in: entries that touch neither scratch
NO_SCRATCH = {"hevc_deblocking_filter_h265_device", "hevcdbk_sao_filter_device_sp"}
# the scratches an entry can be made to use (beside none: the fused kernel, 4:2:0)
ONLY_TMP = {"hevc_deblock_sao_device", "hevc_deblock_sao_device_planes", "hevc_deblock_sao_h265_device", "hevc_deblock_sao_h265_device_planes",
            "hevcdbk_h265_deblock_sao_device_sp", "hevcdbk_h265_deblock_sao_device_sp_fused", "hevcdbk_h265_deblock_sao_device_nv12"}
ONLY_SAO = {"hevcdbk_sao_filter_device_cf", "hevcdbk_sao_filter_device_nox", "hevcdbk_sao_filter_device_g4"}
EITHER = {"hevcdbk_h265_deblock_sao_device" + g for g in ("_cf", "_nox", "_sl", "_g4", "_planes_cf", "_planes_nox", "_planes_sl", "_planes_g4")}
SITES = {(e, "tmp") for e in ONLY_TMP | EITHER} | {(e, "sao") for e in ONLY_SAO | EITHER} | {(e, "both") for e in EITHER}


def no_aslr(cmd):
    """as tests/test_host_frame_sim_cpu.py: ThreadSanitizer's programs run with address randomisation off for that one process"""
    import shutil
    return [shutil.which("setarch"), os.uname().machine, "-R"] + cmd if shutil.which("setarch") else cmd


def tally(out, key):
    return {k: int(n) for k, n in re.findall(r"^%s (\S+) (\d+)$" % key, out, re.M)}


def entries_that_reach_a_scratch():
    """the exported entries of the two sources from which through_scratch or sao_square_params can be reached, by the names that
    occur in the bodies of the functions of the sources and of deblock_host_args.h"""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("deblock_host_h265.cpp", "deblock_host_sp.cpp", "deblock_host_args.h"))
    bodies = {}
    # a definition at the start of a line: its body on the same line, or down to the next closing brace at the start of a line
    for m in re.finditer(r"^(?:inline |static )?(?:int|bool|size_t|void|Gen|unsigned) (\w+)\([^;{]*?\)\s*(?:\{([^\n]*)\}$|\{(.*?)^\})", text, re.M | re.S):
        bodies[m.group(1)] = bodies.get(m.group(1), "") + (m.group(2) or m.group(3) or "")
    reach = {"through_scratch", "sao_square_params"}
    assert reach <= set(bodies)
    grew = True
    while grew:
        grew = False
        for name, body in bodies.items():
            if name not in reach and any(re.search(r"\b%s\(" % r, body) for r in reach):
                reach.add(name)
                grew = True
    return {n for n in reach if n.startswith("hevc")}


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-j4", "-C", DIR, "all", "sanitized"])


def test_every_entry_that_reaches_a_scratch_is_called():
    """the counterpart of test_entry_sim_cpu.test_every_exported_entry_of_the_file_is_called: an entry added to the sources that runs
    the two-launch form or rewrites 4:2:2 parameters is missed here until the program calls it"""
    covered = entries_that_reach_a_scratch()
    assert ONLY_TMP | ONLY_SAO | EITHER | {"hevc_sao_filter_device"} == covered, covered
    sim = open(os.path.join(DIR, "device_stream_sim.cpp")).read()
    called = set(re.findall(r"return (hevc\w+)\(ctx, ", sim))
    named = set(re.findall(r"\"(hevc\w+)\"", sim))
    assert called == named == covered | NO_SCRATCH, (called ^ named, called ^ (covered | NO_SCRATCH))


@pytest.mark.parametrize("program", ["device_stream_sim", "device_stream_sim_diag"])
def test_sessions_hold_their_properties_under_every_scheduler(built, program):
    r = subprocess.run([os.path.join(DIR, program), "check", SEED, str(SESSIONS)], capture_output=True, text=True, timeout=900)
    # the generator first: sessions that do not contend for a scratch prove nothing about its fence
    count = tally(r.stdout, "count")
    assert count["sessions"] == SESSIONS, r.stdout[-3000:] + r.stderr[-2000:]
    assert sum(tally(r.stdout, "scheduler").values()) == SESSIONS and set(tally(r.stdout, "scheduler")) == SCHEDULERS
    ran = {}
    for key, n in tally(r.stdout, "ran").items():
        entry, scratch, sched = key.split("/")
        ran[(entry, scratch, sched)] = n
    covered = entries_that_reach_a_scratch()
    for entry in covered:
        for sched in SCHEDULERS:
            assert sum(n for (e, _, s), n in ran.items() if e == entry and s == sched) >= 50, (entry, sched)
    assert {(e, sc) for (e, sc, _) in ran if sc != "none"} == SITES
    assert all(ran.get((e, sc, s), 0) >= 5 for (e, sc) in SITES for s in SCHEDULERS), ran
    # two calls on different streams use the same scratch with no blocking call between them: in at least half of the sessions
    assert 2 * count["contended"] >= SESSIONS, count
    assert 10 * count["grew"] >= SESSIONS and count["smaller_after_larger"] >= SESSIONS // 10, count
    assert count["first_use_tmp"] >= SESSIONS // 2 and count["first_use_sao"] >= SESSIONS // 2, count
    # every kind of failure inside every entry's use of every scratch
    faults = {}
    for key, n in tally(r.stdout, "fault").items():
        entry, scratch, sched, kind = key.split("/")
        faults[(entry, scratch, sched, kind)] = n
    assert all(sum(n for (e, sc, _, k), n in faults.items() if (e, sc, k) == (entry, scratch, kind)) >= 1 for (entry, scratch) in SITES for kind in FAULTS), faults
    # ... and every kind inside every scratch under every scheduler
    for scratch in ("tmp", "sao", "both"):
        for sched in SCHEDULERS:
            for kind in FAULTS:
                assert sum(n for (_, sc, s, k), n in faults.items() if (sc, s, k) == (scratch, sched, kind)) >= 50, (scratch, sched, kind)
    # the properties
    assert r.returncode == 0 and "\n0 violations\n" in r.stdout and not tally(r.stdout, "violations_by"), r.stdout[-6000:] + r.stderr[-2000:]


@pytest.mark.parametrize("program", ["device_stream_sim_asan", "device_stream_sim_tsan"])
def test_sessions_under_the_sanitizers(built, program):
    cmd = [os.path.join(DIR, program), "check", SEED, str(SANITIZED_SESSIONS)]
    r = subprocess.run(no_aslr(cmd) if program.endswith("tsan") else cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "\n0 violations\n" in r.stdout, r.stdout[-6000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert tally(r.stdout, "count")["sessions"] == SANITIZED_SESSIONS
