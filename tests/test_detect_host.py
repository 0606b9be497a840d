"""The detector's host half (csrc/detect_host.h) on its own: tests/cpp/detect_host_check.cpp compiled with the address and
undefined-behaviour sanitizers and run directly; the balls it prints for its own frames are held against tests/detect_ref.py's
association, bit for bit."""
import os
import subprocess

import numpy as np

import detect_ref as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lcg(s):
    s[0] = (s[0] * 1664525 + 1013904223) & 0xffffffff
    return s[0] >> 8


def test_host_code_under_address_and_ub_sanitizers(tmp_path):
    exe = tmp_path / "detect_host_check"
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "gpismap_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "detect_host_check.cpp"),
                           "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "0", lines[-5:]
    got = [l.split()[1:] for l in lines if l.startswith("B ")]
    # the program's frames through the reference
    o = dr.opts(2, 0.1, gate=0.5, max_missed=3)
    tr = dict(balls=[], t_prev=0.0, held=False, next_id=0)
    s, t, want = [12345], 0.0, []
    for f in range(12):
        t += 0.25
        n = _lcg(s) % 8
        det = []
        for j in range(n):
            c0 = _lcg(s) % 2001 / 1000.0 - 1.0
            c1 = _lcg(s) % 2001 / 1000.0 - 1.0
            det.append(dict(c=[c0, c1], r=0.1, comp=j))
        for b in dr.associate(2, det, t, o, tr):
            vals = np.array([b["c"][0], b["c"][1], b["v"][0], b["v"][1], b["r"]], np.float64).view(np.uint64)
            want.append([str(f), str(b["id"]), str(b["age"]), str(b["missed"]), str(b["comp"])] + ["%016x" % int(v) for v in vals])
    assert len(want) > 30 and any(w[2] not in ("0", "1") for w in want) and any(w[3] != "0" for w in want)
    assert got == want, next((g, w) for g, w in zip(got, want) if g != w)
