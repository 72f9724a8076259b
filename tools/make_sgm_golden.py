#!/usr/bin/env python3
"""Writes tests/golden/sgm/ from the reference's own semi-global matcher.

    python tools/make_sgm_golden.py --reference /path/to/reference [--out tests/golden/sgm]

Runs only where the reference is checked out.  In a temporary directory it writes a stub of the one OpenCV type the
matcher needs and a small main of its own, extracts the matcher's section of the reference's src/stereo_algorithm.cc
between marker lines at run time, compiles the lot with g++ once at -O0 and once at -O2, and runs every case through both.
Only data reaches the repository: cases.json and one .npz per case (input pair and the uint16 map).  Nothing extracted or
compiled is kept, and this file holds no line of the reference.

Refuses to write when the two builds differ, when a float output is not exactly uint16 / disparityFactor, when two pairs
through ONE matcher object differ from fresh-object runs, or when a main case misses its conditions (50-98 % non-zero
pixels, >= 90 % of them within 1 px of the planted disparity)."""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import sgm_util  # noqa: E402

HEADERS = "cstdlib cstring climits cstdio cmath cstdint vector memory new"

STUB = """
namespace cv { struct Mat { int rows, cols; unsigned char* data;
  template <class T> const T* ptr() const { return (const T*)data; } }; }
"""

# (first line starts with, last line starts with) of each range taken from the reference, in order
RANGES = [("template <typename T, std::size_t Alignment", "}; // bpvo"),
          ("#include <limits>", "#include <immintrin.h>"),
          ("class SGMStereo {", "};"),
          ("// Default parameters", "#endif // WITH_GPL_CODE")]

MAIN = r"""
// in: int32 n, rows, cols, D, cap, census radius, window radius, P1, P2, threshold; double factor, weight; n x (left, right)
// out: n x rows*cols float.  mode "reuse": one matcher object for all pairs; "fresh": a new object per pair.
int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int h[10]; double g[2];
  if (fread(h, sizeof(int), 10, f) != 10 || fread(g, sizeof(double), 2, f) != 2) return 4;
  const int n = h[0], rows = h[1], cols = h[2];
  const size_t npix = (size_t)rows * cols;
  std::vector<unsigned char> img(2 * npix * n);
  if (fread(img.data(), 1, img.size(), f) != img.size()) return 5;
  fclose(f);
  const bool reuse = strcmp(argv[3], "reuse") == 0;
  std::vector<float> out(npix * n);
  SGMStereo* m = nullptr;
  for (int i = 0; i < n; ++i) {
    if (!m) {
      m = new SGMStereo();
      m->setDisparityTotal(h[3]);
      m->setDisparityFactor(g[0]);
      m->setDataCostParameters(h[4], h[5], g[1], h[6]);
      m->setSmoothnessCostParameters(h[7], h[8]);
      m->setConsistencyThreshold(h[9]);
    }
    cv::Mat L{rows, cols, img.data() + 2 * npix * i}, R{rows, cols, img.data() + 2 * npix * i + npix};
    m->compute(L, R, out.data() + npix * i);
    if (!reuse) { delete m; m = nullptr; }
  }
  delete m;
  f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), sizeof(float), out.size(), f) != out.size()) return 6;
  fclose(f);
  return 0;
}
"""


def extract(path):
    with open(path) as f:
        lines = f.read().split("\n")
    parts, at = [], 0
    for first, last in RANGES:
        while not lines[at].startswith(first):
            at += 1
        start = at
        while not lines[at].startswith(last):
            at += 1
        end = at if last.startswith("#endif") else at + 1   # the closing #endif stays out
        parts.append("\n".join(lines[start:end]))
        at = end
    return parts


def build(reference, tmp):
    parts = extract(os.path.join(reference, "src", "stereo_algorithm.cc"))
    src = os.path.join(tmp, "sgm_main.cpp")
    with open(src, "w") as f:
        f.write("".join("#include <%s>\n" % h for h in HEADERS.split()))
        f.write(STUB)
        f.write("\n".join(parts))
        f.write(MAIN)
    exes = []
    for opt in ("-O0", "-O2"):
        exe = os.path.join(tmp, "sgm" + opt)
        subprocess.check_call(["g++", opt, "-std=c++14", "-msse4.2", "-mpopcnt", "-w", "-o", exe, src])
        exes.append(exe)
    return exes


def run(exe, tmp, pairs, p, mode):
    rows, cols = pairs[0][0].shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<10i2d", len(pairs), rows, cols, p["numberOfDisparities"], p["sobelCapValue"], p["censusRadius"],
                            p["windowRadius"], p["smoothnessPenaltySmall"], p["smoothnessPenaltyLarge"],
                            p["consistencyThreshold"], p["disparityFactor"], p["censusWeightFactor"]))
        for l, r in pairs:
            f.write(l.tobytes())
            f.write(r.tobytes())
    subprocess.check_call([exe, fin, fout, mode])
    return np.fromfile(fout, np.float32).reshape(len(pairs), rows, cols)


def case_list():
    c = []
    for name, rows, cols, nd in (("main_24x64", 24, 64, 16), ("main_48x128", 48, 128, 32), ("main_96x256", 96, 256, 64),
                                 ("main_376x1241", 376, 1241, 128)):
        c.append(dict(name=name, kind="main", rows=rows, cols=cols, ndisp=nd, params={}))
    c.append(dict(name="odd_37x131", kind="odd", rows=37, cols=131, ndisp=48, params={}))
    c.append(dict(name="edge_cols_eq_d", kind="edge", rows=20, cols=64, ndisp=64, params={}))
    c.append(dict(name="edge_rows_3", kind="edge", rows=3, cols=80, ndisp=16, params={}))
    for name, params in (("cap127", dict(sobelCapValue=127)), ("census1", dict(censusRadius=1)),
                         ("window0", dict(windowRadius=0)), ("window5", dict(windowRadius=5)),
                         ("window9", dict(windowRadius=9)), ("weight1", dict(censusWeightFactor=1.0)),
                         ("penalty_0_1", dict(smoothnessPenaltySmall=0, smoothnessPenaltyLarge=1)),
                         ("penalty_3000_12000", dict(smoothnessPenaltySmall=3000, smoothnessPenaltyLarge=12000)),
                         ("threshold0", dict(consistencyThreshold=0)), ("threshold3", dict(consistencyThreshold=3)),
                         ("factor16", dict(disparityFactor=16.0)), ("factor2048", dict(disparityFactor=2048.0)),
                         ("cap127_weight1_window9", dict(sobelCapValue=127, censusWeightFactor=1.0, windowRadius=9))):
        c.append(dict(name="param_" + name, kind="param", rows=30, cols=96, ndisp=32, params=params))
    for i, case in enumerate(c):
        case["seed"] = 7100 + i
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "sgm"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    written, done = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exes = build(args.reference, tmp)
        for case in case_list():
            p = sgm_util.params_of(case)
            left, right, planted = sgm_util.make_pair(case["rows"], case["cols"], case["ndisp"], case["seed"])
            other = sgm_util.make_pair(case["rows"], case["cols"], case["ndisp"], case["seed"] + 1000)[:2]
            pairs = [(left, right), other, (left, right)]
            outs = [run(e, tmp, pairs, p, "reuse") for e in exes]
            if outs[0].tobytes() != outs[1].tobytes():
                sys.exit("%s: the -O0 and -O2 builds differ" % case["name"])
            fresh = run(exes[1], tmp, pairs, p, "fresh")
            if fresh.tobytes() != outs[1].tobytes():
                sys.exit("%s: one matcher object reused differs from fresh objects" % case["name"])
            disp = outs[1][0]
            scaled = disp.astype(np.float64) * p["disparityFactor"]
            u16 = scaled.astype(np.uint16)
            if not (scaled == u16).all() or sgm_util.float_map(u16, p["disparityFactor"]).tobytes() != disp.tobytes():
                sys.exit("%s: the float output is not uint16 / disparityFactor" % case["name"])
            nz = u16 != 0
            within = np.abs(disp[nz] - planted[nz]) <= 1.0
            case["input_sha256"] = sgm_util.sha256(left, right)
            case["disparity_sha256"] = sgm_util.sha256(disp)
            case["disp_scaled_sha256"] = sgm_util.sha256(u16)
            case["nonzero_share"] = round(float(nz.mean()), 4)
            case["within_1px_share"] = round(float(within.mean()) if nz.any() else 0.0, 4)
            if case["kind"] == "main" and not (0.5 <= nz.mean() <= 0.98 and within.mean() >= 0.9):
                sys.exit("%s misses the conditions on main cases: non-zero %.3f, within 1 px %.3f"
                         % (case["name"], nz.mean(), within.mean()))
            if case["rows"] * case["cols"] <= 96 * 256:
                case["file"] = case["name"] + ".npz"
                written[case["file"]] = dict(left=left, right=right, disp_scaled=u16)
            else:
                case["file"] = None
                case["rows_file"] = case["name"] + "_rows.npz"
                idx = np.arange(0, case["rows"], 16, dtype=np.int32)
                written[case["rows_file"]] = dict(row_index=idx, disp_rows=u16[idx])
            print("%-28s non-zero %.3f  within 1 px %.3f" % (case["name"], case["nonzero_share"], case["within_1px_share"]))
            done.append(case)
    # every case passed: write
    for name, arrays in written.items():
        np.savez_compressed(os.path.join(args.out, name), **arrays)
    with open(os.path.join(args.out, "cases.json"), "w") as f:
        json.dump(dict(defaults=sgm_util.DEFAULTS, cases=done), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
