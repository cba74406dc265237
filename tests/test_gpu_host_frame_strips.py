"""What ties the CPU model of the host-frame operators (tests/host_frame_sim) to the card: the strips hevc_deblocking_filter cuts a
large pageable frame into on an MI355X are, entry for entry, the strips the same host source cuts it into against the modelled HIP
runtime -- so the strip pipeline the 3000 CPU cases walk through is the one that runs here -- and the frames come out bit-exact.
Three frames of a few milliseconds each.  There is deliberately no GPU case of a partly registered plane or of a failing launch: a
wrong fix would fault the card, and the CPU cases show both."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SIM = os.path.join(ROOT, "tests", "host_frame_sim")


@pytest.fixture(scope="module")
def ctx():
    from gpu_video_codec_amd import deblock
    c = deblock.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sim():
    subprocess.check_call(["make", "-s", "-C", SIM, "host_frame_sim"])
    return os.path.join(SIM, "host_frame_sim")


def modelled_strips(sim, w, h, sb, chroma, pitched=False):
    """the model's table for a pageable frame on a large-BAR device, rows tight or 16 samples apart from tight"""
    r = subprocess.run([sim, "strips", str(w), str(h), str(sb), str(int(chroma)), "1", str(int(pitched))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [tuple(int(v) for v in m) for m in re.findall(r"^strip (\d+) (\d+) (\d+) (\d+)$", r.stdout, re.M)]


def traced_strips(ctx):
    return [(s["plane"], s["row_begin"], s["row_end"], s["bytes"]) for s in ctx.last_frame_trace()]


def test_pageable_8bit_luma_in_three_strips(ctx, oracle, sim):
    from gpu_video_codec_amd import synth
    y = synth.blocky_plane(1024, 1032, seed=91)
    got = y.copy()
    ctx.filter_frame(got, qp=33)
    want = modelled_strips(sim, 1024, 1032, 1, False)
    assert len(want) == 3 and traced_strips(ctx) == want
    assert np.array_equal(got, oracle.filter_plane(y, 33))


def test_10bit_luma_in_pitched_rows(ctx, oracle, sim):
    from gpu_video_codec_amd import synth
    y = synth.blocky_plane(256, 4104, seed=92, bit_depth=10)
    buf = np.full((4104, 256 + 16), 0x0155, np.uint16)
    view = buf[:, :256]
    view[:] = y
    ctx.filter_frame(view, qp=31, bit_depth=10)
    want = modelled_strips(sim, 256, 4104, 2, False, pitched=True)
    assert len(want) >= 3 and traced_strips(ctx) == want
    assert np.array_equal(view, oracle.filter_plane(y, 31, bit_depth=10))
    assert (buf[:, 256:] == 0x0155).all()


def test_8bit_yuv420_1920x1088(ctx, oracle, sim):
    from gpu_video_codec_amd import synth
    y, u, v = synth.blocky_yuv420(1920, 1088, seed=93)
    got = [p.copy() for p in (y, u, v)]
    ctx.filter_frame(*got, qp=36)
    want = modelled_strips(sim, 1920, 1088, 1, True)
    assert {p for p, _, _, _ in want} == {0, 1, 2} and traced_strips(ctx) == want
    assert oracle.join_yuv420(*got) == oracle.filter_yuv420(oracle.join_yuv420(y, u, v), 1920, 1088, 36)
