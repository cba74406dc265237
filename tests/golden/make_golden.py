#!/usr/bin/env python3
"""Generate the golden vectors in tests/golden/ from the REFERENCE's own CPU implementation.

Run only in the build container (needs /root/reference and oracle/_ref, see oracle/Makefile):

    make -C oracle ref && python tests/golden/make_golden.py

What it writes (all data, no reference source):
  * the three bundled input frames, copied byte-for-byte as fixtures,
  * <name>_qp<QP>.ref.yuv     -- full reference output for the three main.cu configurations
                                 (main.cu:112-133: image1 QP30, image2 QP30, mother-daughter QP35),
  * manifest.json             -- sha256 of input, of the whole filtered file and of its luma
                                 plane for every (image, QP, bS variant); bS variants are the
                                 default pattern and LCG-seeded luma bS in {0,1,2}
                                 (oracle.lcg_bs: s = s*1664525+1013904223, (s>>16)%3, vert then hor),
  * synth_*.json entries      -- sha256 of reference outputs on seeded synthetic 4:2:0 frames
                                 (gpu_video_codec_amd.synth.blocky_yuv420), small and 4K,
  * ref_fresh.json            -- sha256 of reference outputs on the hard seeded inputs of fresh_cases()
                                 and the reference constructor's return codes on the files of ERROR_CASES
                                 (tests/test_oracle.py checks the restatement against both),
  * ref_boundaries.json       -- sha256 of input and reference output of the boundary frames of boundary_cases():
                                 segments solved onto every decision threshold (tests/ref_vectors.py), with their luma
                                 bS override (tests/test_ref_boundaries_cpu.py checks the restatement against it).

    python tests/golden/make_golden.py --boundaries   rewrites ref_boundaries.json alone.
"""
import hashlib
import json
import os
import shutil
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from gpu_video_codec_amd import synth  # noqa: E402
from oracle import oracle  # noqa: E402

REF_DIR = "/root/reference/hevc_deblocking_filter"
IMAGES = {
    "image1": ("image1_352x288_yv12.yuv", 352, 288, 30),
    "mother-daughter": ("mother-daughter_352x288_yv12.yuv", 352, 288, 35),
    "image2": ("image2_768x576.yuv", 768, 576, 30),
}
QPS = [0, 17, 18, 22, 27, 30, 32, 35, 37, 42, 47, 51, 60]
SEEDS = [1, 2, 12345]
SYNTH = [(64, 48, 7), (352, 288, 3), (3840, 2160, 1)]  # (w, h, seed)
SYNTH_QPS = [27, 32, 45]


def sha(b):
    return hashlib.sha256(b).hexdigest()


def fresh_cases():
    """Seeded 4:2:0 frames with hard content (noise patches, saturated areas) at sizes and QPs no other fixture covers:
    yields (w, h, qp, bs_seed, yuv bytes, vert bS, hor bS); bS None = the reference's default pattern."""
    import numpy as np
    rng = np.random.default_rng(11)
    for (w, h) in [(16, 16), (32, 16), (16, 48), (64, 64), (176, 144), (400, 240)]:
        for qp in (20, 27, 33, 40, 51):
            y, u, v = synth.blocky_yuv420(w, h, seed=int(rng.integers(1, 1 << 30)))
            y = y.copy()
            y[: h // 4, : w // 4] = rng.integers(0, 256, (h // 4, w // 4), dtype=np.uint8)
            y[h // 2:, w // 2:] = 255
            y[h // 2:, : w // 8] = 0
            buf = oracle.join_yuv420(y, u, v)
            for seed in (None, 9):
                vb = hb = None
                if seed is not None:
                    vb, hb = oracle.lcg_bs(w, h, seed)
                yield w, h, qp, seed, buf, vb, hb


# constructor error cases (cpu.h:43-48): name -> (file size in bytes, width, height)
ERROR_CASES = {"short_file": (100, 352, 288), "dimensions_not_multiple_of_8": (3 * 20 * 20 // 2, 20, 20)}


def record_fresh():
    import ctypes as C
    import tempfile
    cases = [{"width": w, "height": h, "qp": qp, "bs_seed": seed, "input_sha256": sha(buf),
              "sha256": sha(oracle.ref_filter_yuv420(buf, w, h, qp, vb, hb, threads=1))}
             for (w, h, qp, seed, buf, vb, hb) in fresh_cases()]
    errors = {}
    with tempfile.TemporaryDirectory() as d:
        for name, (size, w, h) in ERROR_CASES.items():
            p = os.path.join(d, name + ".yuv")
            with open(p, "wb") as fh:
                fh.write(b"\0" * size)
            errors[name] = oracle.ref().ref_frame_create(C.byref(C.c_void_p()), p.encode(), w, h, 30)
    with open(os.path.join(HERE, "ref_fresh.json"), "w") as fh:
        json.dump({"cases": cases, "constructor_errors": errors}, fh, indent=1)
    print("wrote", os.path.join(HERE, "ref_fresh.json"))


# boundary frames: 8-bit 4:2:0, scalar QP, one luma wave each (tests/ref_vectors.py); sizes multiples of 16
BOUNDARY_SIZES = [(16, 16), (48, 32), (112, 48), (528, 48)]
BOUNDARY_QPS = [18, 27, 35, 42, 51]


def boundary_cases():
    """Seeded 8-bit 4:2:0 frames whose luma segments are solved onto the reference's decision thresholds, range extremes and
    picture border (luma bS override: vertical-only, horizontal-only or mixed waves) and whose chroma segments sit on the
    +-tc clips and Clip2 under the default chroma bS: yields (w, h, qp, wave, yuv bytes, vert bS, hor bS)."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ref_vectors as rv
    rng = np.random.default_rng(29)
    for i, (w, h) in enumerate(BOUNDARY_SIZES):
        for j, qp in enumerate(BOUNDARY_QPS):
            wave = rv.WAVES[(i + j) % 3]
            y, u, v, vb, hb = rv.boundary_frame(w, h, qp, wave, rng)
            yield w, h, qp, wave, oracle.join_yuv420(y, u, v), vb, hb


def record_boundaries():
    cases = [{"width": w, "height": h, "qp": qp, "wave": wave, "input_sha256": sha(buf),
              "sha256": sha(oracle.ref_filter_yuv420(buf, w, h, qp, vb, hb, threads=1))}
             for (w, h, qp, wave, buf, vb, hb) in boundary_cases()]
    with open(os.path.join(HERE, "ref_boundaries.json"), "w") as fh:
        json.dump({"cases": cases}, fh, indent=1)
    print("wrote", os.path.join(HERE, "ref_boundaries.json"))


def main():
    assert oracle.have_ref(), "build oracle/_ref first (make -C oracle ref)"
    man = {"images": {}, "synth": []}
    for name, (fn, w, h, main_qp) in IMAGES.items():
        shutil.copyfile(os.path.join(REF_DIR, fn), os.path.join(HERE, fn))
        buf = open(os.path.join(HERE, fn), "rb").read()
        ent = {"file": fn, "width": w, "height": h, "main_qp": main_qp, "input_sha256": sha(buf), "cases": []}
        for qp in QPS:
            for seed in [None] + SEEDS:
                if seed is not None and qp not in (30, 37):
                    continue
                vb = hb = None
                if seed is not None:
                    vb, hb = oracle.lcg_bs(w, h, seed)
                out = oracle.ref_filter_yuv420(buf, w, h, qp, vb, hb, threads=1)
                ent["cases"].append({"qp": qp, "bs_seed": seed, "sha256": sha(out), "luma_sha256": sha(out[: w * h])})
                if seed is None and qp == main_qp:
                    with open(os.path.join(HERE, "%s_qp%d.ref.yuv" % (name, qp)), "wb") as fh:
                        fh.write(out)
        man["images"][name] = ent
    for (w, h, seed) in SYNTH:
        y, u, v = synth.blocky_yuv420(w, h, seed=seed, frame=0)
        buf = oracle.join_yuv420(y, u, v)
        for qp in SYNTH_QPS:
            for bs_seed in (None, 5):
                vb = hb = None
                if bs_seed is not None:
                    vb, hb = oracle.lcg_bs(w, h, bs_seed)
                out = oracle.ref_filter_yuv420(buf, w, h, qp, vb, hb, threads=1)
                man["synth"].append({"width": w, "height": h, "seed": seed, "frame": 0, "qp": qp, "bs_seed": bs_seed,
                                     "input_sha256": sha(buf), "sha256": sha(out), "luma_sha256": sha(out[: w * h])})
    with open(os.path.join(HERE, "manifest.json"), "w") as fh:
        json.dump(man, fh, indent=1)
    print("wrote", os.path.join(HERE, "manifest.json"))
    record_fresh()
    record_boundaries()


if __name__ == "__main__":
    if sys.argv[1:] == ["--boundaries"]:
        assert oracle.have_ref(), "build oracle/_ref first (make -C oracle ref)"
        record_boundaries()
    else:
        main()
