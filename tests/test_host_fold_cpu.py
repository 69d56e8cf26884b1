"""gn_fold8_rows (csrc/gn_math.h), the host's side of the fold of a host-driven single-GPU pass, compiled as plain host C++: it
adds the 8 group rows in the order the emitting block of ticket_fold_emit (csrc/pass_device.h) adds them,
((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)), in IEEE double -- bit for bit against that expression in NumPy float64, on
rows with signed zeros, infinities, denormals, pairs that cancel and magnitudes 300 decades apart.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rows_under_test():
    rng = np.random.default_rng(17)
    tiny = np.float64(5e-324)
    sets = [rng.normal(0.0, 1.0, (8, 32)),
            rng.normal(0.0, 1.0, (8, 32)) * 10.0 ** rng.integers(-300, 300, (8, 32)),
            np.zeros((8, 32)), -np.zeros((8, 32))]
    special = np.zeros((8, 32))
    special[:, 0] = [0.0, -0.0, 0.0, -0.0, -0.0, -0.0, 0.0, 0.0]
    special[:, 1] = -0.0                                                # all negative zeros: the sum is -0
    special[:, 2] = [np.inf, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
    special[:, 3] = [np.inf, 1.0, 2.0, 3.0, -np.inf, 5.0, 6.0, 7.0]     # inf - inf: NaN
    special[:, 4] = [tiny, tiny, -tiny, tiny, 2 * tiny, -tiny, tiny, tiny]
    special[:, 5] = [1e308, 1e308, -1e308, -1e308, 1.0, 2.0, 3.0, 4.0]  # both pairs overflow, to opposite signs: NaN, where a left-to-right sum gives 10
    special[:, 6] = [1.0, 1e-17, -1.0, 1e-17, 1e16, 1.0, -1e16, 1.0]    # cancelling pairs: the order decides the result
    special[:, 7] = [1e16, 1.0, 1.0, -1e16, 3.0, 1e-300, -3.0, 2.2250738585072014e-308]
    special[:, 8] = [-np.inf, -1.0, 0.0, 1.0, 2.0, 3.0, 4.0, -np.inf]
    special[:, 9:] = rng.normal(0.0, 1e3, (8, 23)) * np.where(rng.random((8, 23)) < 0.5, 1.0, 1e-12)
    return sets + [special]


def restated(v):
    with np.errstate(all="ignore"):
        return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not installed")
def test_host_fold_is_the_device_order(tmp_path):
    sets = rows_under_test()
    src = r"""
#include <stdio.h>
#include <string.h>
#include <stdint.h>
#include "gn_math.h"
int main() {
    double rows[256], tot[32];
    uint64_t w;
    for (;;) {
        for (int i = 0; i < 256; ++i) {
            if (scanf("%llx", (unsigned long long *)&w) != 1) return 0;
            memcpy(&rows[i], &w, 8);
        }
        for (int k = 0; k < 32; ++k) tot[k] = -7.0;
        gn_fold8_rows(rows, tot, 29);
        for (int k = 0; k < 32; ++k) { memcpy(&w, &tot[k], 8); printf("%llx ", (unsigned long long)w); }
        printf("\n");
    }
}
"""
    (tmp_path / "t.cpp").write_text(src)
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(REPO, "point_cloud_registration_amd", "csrc"),
                    str(tmp_path / "t.cpp"), "-o", str(tmp_path / "t")], check=True, capture_output=True)
    text = "\n".join(" ".join("%x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in s.reshape(-1)) for s in sets)
    out = subprocess.run([str(tmp_path / "t")], input=text, capture_output=True, text=True, check=True).stdout.strip().splitlines()
    assert len(out) == len(sets)
    for s, line in zip(sets, out):
        got = np.array([struct.unpack("<d", struct.pack("<Q", int(x, 16)))[0] for x in line.split()])
        want = restated(s)
        assert np.array_equal(got[29:], [-7.0] * 3)                                # 29 components, no more
        nan = np.isnan(want[:29])
        assert np.array_equal(np.isnan(got[:29]), nan)
        # bit for bit, the sign of a zero included
        assert np.array_equal(got[:29][~nan].view(np.uint64), want[:29][~nan].view(np.uint64))
    sp = restated(sets[-1])
    # (the special columns are what their comments say)
    assert np.signbit(sp[1]) and sp[1] == 0.0 and not np.signbit(sp[0]) and np.isnan(sp[3]) and np.isinf(sp[2]) and np.isnan(sp[5])
    assert sp[4] == 5 * 5e-324 and sp[6] == 0.0                  # (the exact sum of column 6 is 2 + 2e-17: the order decides)


def test_the_library_is_built_without_reassociation():
    """the host adds in the order written only if no flag lets the compiler reorder float64 adds"""
    mk = open(os.path.join(REPO, "point_cloud_registration_amd", "csrc", "Makefile")).read()
    for flag in ("-ffast-math", "-Ofast", "-fassociative-math", "-funsafe-math-optimizations", "-ffp-model=fast"):
        assert flag not in mk, flag
