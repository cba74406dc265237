"""The C-ABI entries of csrc/deblock_host_h265.cpp without a GPU (tests/entry_sim: the two real host sources linked against stubs of
the HIP runtime and of the kernel launchers).  Over operands made from a seed -- a valid call with zero, one or two things wrong
with it -- the program calls every entry and compares, as return code plus error text plus the trace of what was enqueued, the
generations of an entry where include/hevc_deblock.h promises that they are the same call:

  * an _sl entry without slice_offsets and the _nox (_cf) entry;
  * a _g4 entry on planes sized in multiples of 8 and the _sl (_nox) entry;
  * a _nox entry without borders and the _cf entry;
  * a _cf entry with 4:2:0 and square CTBs and the original entry, where neither was refused before the launch.

Of every call it asks that nothing is enqueued after a refusal, and that the last launch into the context's scratch for 4:2:2 SAO
parameters that was enqueued (parameters or border bytes) is followed by the record of the event that fences it, whatever the
launches after it returned, in the SAO pass entries as in the deblocking + SAO entries.  Both builds of the host source, product
and diagnostic."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "entry_sim")
CASES = 3000
IDENTITIES = 16
ENTRIES = 29


@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", DIR, "all"])


@pytest.mark.parametrize("program", ["entry_sim", "entry_sim_diag"])
def test_generations_of_an_entry_agree_and_refusals_enqueue_nothing(built, program):
    r = subprocess.run([os.path.join(DIR, program), "check", "20251", str(CASES)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "\n0 violations\n" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    ran = dict(re.findall(r"^cases (\S+) (\d+)$", r.stdout, re.M))
    assert len(ran) == ENTRIES and all(int(n) == CASES for n in ran.values()), ran
    compared = {k: int(n) for k, n in re.findall(r"^compared (.+) (\d+)$", r.stdout, re.M)}
    assert len(compared) == IDENTITIES, compared
    # an identity that holds for every operand set is compared on all of them; one with a condition on a good share of them
    assert all(n >= CASES // 20 for n in compared.values()), compared
    assert sum(n == CASES for n in compared.values()) == 6, compared


def test_every_exported_entry_of_the_file_is_called():
    """the entries the program calls are the file's exported functions, less the two host-frame operators (and the two bS array sizes
    under one name)"""
    src = open(os.path.join(ROOT, "gpu_video_codec_amd", "csrc", "deblock_host_h265.cpp")).read()
    exported = set(re.findall(r"^(?:int|size_t) (hevc\w+)\(", src, re.M))
    sim = open(os.path.join(DIR, "entry_sim.cpp")).read()
    called = set(re.findall(r"^    E\((\w+),", sim, re.M))
    frame_operators = {"hevc_deblocking_filter_h265", "hevcdbk_h265_filter_frame_cf"}
    sizes = {"hevcdbk_h265_num_vert_bs", "hevcdbk_h265_num_hor_bs"}
    assert exported - frame_operators - sizes == called - {"hevcdbk_h265_num_bs"}
    assert "hevcdbk_h265_num_bs" in called and all(s in sim for s in sizes)
