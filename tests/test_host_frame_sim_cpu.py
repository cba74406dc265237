"""The host-frame operators of csrc/deblock_host.cpp and csrc/deblock_host_h265.cpp without a GPU (tests/host_frame_sim: the two real host
sources linked against a model of the HIP runtime that defers every operation and runs it inside a later HIP call chosen by an eager, a
lazy or a seeded random scheduler, with memory kinds, access checks and injected failures).  Cases made from a seed -- entry, transport,
memory kind of every plane, operands, copying threads, frames in flight -- must leave every sample as the marker transform of its
input, every row written once, no access outside an allocation, every stream empty on return (after an injected failure too), the
planes row by row either input or result after a failure, a strip record that tiles every plane, and a context that works on.
Product and diagnostic build of the host sources, and both under AddressSanitizer + UBSan and under ThreadSanitizer; all stand-alone
programs."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "host_frame_sim")
SEED = "20261"
CASES = 3000
SANITIZED_CASES = 300
ENTRIES = {"hevc_deblocking_filter", "hevc_deblocking_filter_sequence", "hevcdbk_filter_yuv_file", "hevc_deblocking_filter_h265",
           "hevcdbk_h265_filter_frame_cf"}
TRANSPORTS = {"small_direct", "small_staged", "strips_bar_push+d2h", "strips_bar_push+kout_caller", "strips_bar_push+kout_ring",
              "strips_h2d+d2h", "strips_h2d+kout_caller", "strips_h2d+kout_ring", "sequence_chunks", "sequence_bar_push", "sequence_dma",
              "file_chunks", "h265_bar_push", "h265_dma"}
# what only the diagnostic build's knobs reach: small frames through DMA copies, kernels reading the page-locked strip themselves
DIAG_TRANSPORTS = {"small_dma", "strips_direct_in+kout_caller", "strips_direct_in+kout_ring"}
SCHEDULERS = {"eager", "lazy", "random"}
# the kinds of HIP call a case makes fail (one kind per case, at each of its calls in turn), and the kinds each entry makes at all
FAULTS = {"launch", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipEventRecord", "hipStreamWaitEvent", "hipEventQuery", "hipMalloc", "hipHostMalloc",
          "hipExtMallocWithFlags"}
H265_FAULTS = {"launch", "hipMemcpyAsync", "hipEventRecord", "hipMalloc", "hipHostMalloc", "hipExtMallocWithFlags"}
ENTRY_FAULTS = {"hevc_deblocking_filter": FAULTS, "hevc_deblocking_filter_sequence": FAULTS,
                "hevcdbk_filter_yuv_file": {"launch", "hipMemcpyAsync", "hipMalloc", "hipHostMalloc"},
                "hevc_deblocking_filter_h265": H265_FAULTS, "hevcdbk_h265_filter_frame_cf": H265_FAULTS}


def no_aslr(cmd):
    """ThreadSanitizer refuses to start ("unexpected memory mapping") where the kernel places mappings with more random bits than its
    shadow layout expects: its programs run with address randomisation off for that one process"""
    import shutil
    return [shutil.which("setarch"), os.uname().machine, "-R"] + cmd if shutil.which("setarch") else cmd


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-j4", "-C", DIR, "all", "sanitized"])


def tally(out, key):
    return {k: int(n) for k, n in re.findall(r"^%s (\S+) (\d+)$" % key, out, re.M)}


@pytest.mark.parametrize("program", ["host_frame_sim", "host_frame_sim_diag"])
def test_cases_hold_their_properties_under_every_scheduler(built, program):
    r = subprocess.run([os.path.join(DIR, program), "check", SEED, str(CASES)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "\n0 violations\n" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    ran, refused = tally(r.stdout, "ran"), tally(r.stdout, "refused")
    assert set(ran) == ENTRIES and all(n >= 50 for n in ran.values()), ran
    assert all(10 * refused.get(e, 0) < ran[e] + refused.get(e, 0) for e in ENTRIES), (ran, refused)
    assert sum(ran.values()) + sum(refused.values()) == CASES
    transports = tally(r.stdout, "transport")
    want = TRANSPORTS | (DIAG_TRANSPORTS if program.endswith("_diag") else set())
    assert set(transports) == want and all(n >= 50 for n in transports.values()), transports
    schedulers = tally(r.stdout, "scheduler")
    assert set(schedulers) == SCHEDULERS and all(n >= 50 for n in schedulers.values()), schedulers
    faults = tally(r.stdout, "fault")
    assert {k for k in faults if "/" not in k} == FAULTS and all(faults[k] >= 50 for k in FAULTS), faults
    per_entry = {e: {k.split("/")[1]: n for k, n in faults.items() if k.startswith(e + "/")} for e in ENTRIES}
    assert all(set(per_entry[e]) == ENTRY_FAULTS[e] and min(per_entry[e].values()) >= 5 for e in ENTRIES), per_entry


@pytest.mark.parametrize("program", ["host_frame_sim_asan", "host_frame_sim_tsan"])
def test_cases_under_the_sanitizers(built, program):
    """the crew's threads are real: a kernel operation that reads a strip before its copy-in group was waited for is a reported race as
    well as a mismatch"""
    cmd = [os.path.join(DIR, program), "check", SEED, str(SANITIZED_CASES)]
    r = subprocess.run(no_aslr(cmd) if program.endswith("tsan") else cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "\n0 violations\n" in r.stdout, r.stdout[-6000:] + r.stderr[-3000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    assert sum(tally(r.stdout, "ran").values()) + sum(tally(r.stdout, "refused").values()) == SANITIZED_CASES


@pytest.mark.parametrize("program", ["host_frame_sim", "host_frame_sim_diag"])
def test_thread_creation_failing_inside_a_call_is_an_error_code(built, program):
    """the k-th thread of the crew does not start (k = 1, 2, 3 of a crew of 3 threads beside the caller): the call returns
    HEVCDBK_ERR_NOMEM with the frame untouched, the process lives, and the next call on the context succeeds"""
    r = subprocess.run([os.path.join(DIR, program), "crewfail"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "\n0 violations\n" in "\n" + r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_calls_listing_is_a_stable_fingerprint(built):
    """`calls SEED N`: one line per case -- the case, the return code of its fault-free call, how often it made each kind of HIP call
    (all but hipEventQuery, whose count is the number of polls), its blocking calls and its kernel operations -- and the same lines from
    two runs, the crew's threads real: what two builds of the host sources (a commit and its parent) can be compared by"""
    runs = [subprocess.run([os.path.join(DIR, "host_frame_sim"), "calls", SEED, "200"], capture_output=True, text=True, timeout=300) for _ in range(2)]
    assert all(r.returncode == 0 for r in runs), runs[0].stderr[-2000:] + runs[1].stderr[-2000:]
    lines = runs[0].stdout.splitlines()
    assert len(lines) == 200 and len({ln.split(" ")[1] for ln in lines}) == 200  # "calls seed=... ": every case once
    kinds = FAULTS - {"hipEventQuery"}
    for ln in lines:
        assert re.match(r"calls seed=\d+ hevc", ln) and re.search(r" rc=-?\d+ ", ln) and "hipEventQuery" not in ln, ln
        assert all(re.search(r" %s=\d+( |$)" % k, ln) for k in kinds | {"blocking", "writes"}), ln
    assert runs[0].stdout == runs[1].stdout


STRIP_SHAPES = [(1024, 1032, 1, 0), (256, 4104, 2, 0), (1920, 1088, 1, 1)]


@pytest.mark.parametrize("shape", STRIP_SHAPES)
def test_strip_table_does_not_depend_on_the_bar(built, shape):
    """the strips of a pageable frame (what tests/test_gpu_host_frame_strips.py compares the card's own record with) are the same
    whether the frame goes in through the BAR or through ring + DMA and whether its rows are tight or pitched, and tile every plane"""
    tables = []
    for bar, pitched in (("1", "0"), ("0", "0"), ("1", "1"), ("0", "1")):
        r = subprocess.run([os.path.join(DIR, "host_frame_sim"), "strips"] + [str(v) for v in shape] + [bar, pitched], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        tables.append([tuple(int(v) for v in m) for m in re.findall(r"^strip (\d+) (\d+) (\d+) (\d+)$", r.stdout, re.M)])
    assert all(t == tables[0] for t in tables[1:]) and len(tables[0]) >= 3
    w, h, sb, chroma = shape
    for plane in range(3 if chroma else 1):
        rows = [(a, b) for p, a, b, _ in tables[0] if p == plane]
        ph = h // 2 if plane else h
        assert rows[0][0] == 0 and rows[-1][1] == ph and all(x[1] == y[0] for x, y in zip(rows, rows[1:]))


def test_every_host_frame_entry_of_both_sources_is_called():
    """the counterpart of test_entry_sim_cpu.test_every_exported_entry_of_the_file_is_called: the entries that take a frame in host
    memory or a file of frames are the five the program calls, and the one it names as out of scope (a model several contexts share)"""
    csrc = os.path.join(ROOT, "gpu_video_codec_amd", "csrc")
    src = open(os.path.join(csrc, "deblock_host.cpp")).read() + open(os.path.join(csrc, "deblock_host_h265.cpp")).read()
    entries = set()
    for name, params in re.findall(r"^(?:extern \"C\" )?int (hevc\w+)\(([^)]*)\)\s*\{", src, re.M | re.S):
        if "hevcdbk_frame *" in params or "in_name" in params:
            entries.add(name)
    sim = open(os.path.join(DIR, "host_frame_sim.cpp")).read()
    called = set(re.findall(r"\b(hevc\w+)\(ctx, (?:&f\.frames|f\.frames|f\.in)", sim))
    out_of_scope = {"hevcdbk_filter_yuv_file_multi", "hevcdbk_execute_gpu"}  # several contexts; a wrapper that creates its own context
    assert called == ENTRIES
    assert entries - out_of_scope == called, (entries, called)
    assert "hevcdbk_filter_yuv_file_multi" in open(os.path.join(DIR, "hip_model.h")).read()
