"""float32 / complex64 / complex128 flat table, CPU side: the native symbols exist, the binding keeps SWIG's
overload errors, and scalar.hpp divides exactly like the reference's compiled complex division."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import pyamg_amd
from pyamg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ENTRIES = ["gauss_seidel", "bsr_gauss_seidel", "jacobi", "bsr_jacobi", "gauss_seidel_indexed", "jacobi_ne",
           "gauss_seidel_ne", "gauss_seidel_nr", "block_jacobi", "block_gauss_seidel", "overlapping_schwarz_csr",
           "csr_matvec", "bsr_matvec"]


def test_typed_symbols_resolve():
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = ["amgcore_%s_%s" % (e, s) for e in ENTRIES for s in ("f32", "c64", "c128")]
    assert len(names) == 39
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


@pytest.mark.parametrize("dt", [np.float32, np.complex64, np.complex128])
def test_typed_overload_errors_like_swig(dt):
    core = pyamg_amd.amg_core
    Ap = np.array([0, 1, 2], dtype=np.intc)
    Aj = np.array([0, 1], dtype=np.intc)
    Ax = np.array([2.0, 2.0], dtype=dt)
    other = np.complex128 if dt != np.complex128 else np.float32
    with pytest.raises(NotImplementedError):     # mixed value dtypes
        core.gauss_seidel(Ap, Aj, Ax, np.zeros(2, dtype=other), np.ones(2, dtype=dt), 0, 2, 1)
    with pytest.raises(NotImplementedError):
        core.jacobi(Ap, Aj, Ax, np.zeros(2, dt), np.ones(2, dt), np.zeros(2, dt), 0, 2, 1, np.ones(1, other))
    with pytest.raises(NotImplementedError):     # int64 indices
        core.gauss_seidel(Ap.astype(np.int64), Aj, Ax, np.zeros(2, dt), np.ones(2, dt), 0, 2, 1)
    with pytest.raises(NotImplementedError):
        core.csr_matvec(2, 2, Ap, Aj.astype(np.int64), Ax, np.ones(2, dt), np.zeros(2, dt))
    with pytest.raises(NotImplementedError):     # values of an unsupported dtype
        core.csr_matvec(2, 2, Ap, Aj, np.ones(2, np.float16), np.ones(2, np.float16), np.zeros(2, np.float16))
    with pytest.raises(TypeError):               # strided
        core.gauss_seidel(Ap, Aj, Ax, np.zeros(4, dt)[::2], np.ones(2, dt), 0, 2, 1)
    with pytest.raises(TypeError):
        core.csr_matvec(2, 2, Ap, Aj, Ax, np.ones(4, dt)[::2], np.zeros(2, dt))


DIV_PROBE = r"""
#include "scalar.hpp"
#include <cstdio>
#include <vector>
using namespace amg::sc;
template <class C> int run(const char *in, const char *out, long n)
{
    std::vector<C> v(2 * n), r(n);
    FILE *f = std::fopen(in, "rb");
    if (!f || std::fread(v.data(), sizeof(C), 2 * n, f) != (size_t)(2 * n)) return 1;
    std::fclose(f);
    for (long i = 0; i < n; ++i) r[i] = div(v[2 * i], v[2 * i + 1]);
    f = std::fopen(out, "wb");
    std::fwrite(r.data(), sizeof(C), n, f);
    std::fclose(f);
    return 0;
}
int main(int argc, char **argv)
{
    long n = std::atol(argv[4]);
    return argv[1][0] == 's' ? run<c64>(argv[2], argv[3], n) : run<c128>(argv[2], argv[3], n);
}
"""


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ is not installed")
def test_scalar_header_reproduces_the_division_sweep(tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("#include <cstdlib>\n" + DIV_PROBE)
    exe = tmp_path / "probe"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I",
                    os.path.join(ROOT, "pyamg_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    z = np.load(os.path.join(GOLDEN, "division_dtypes.npz"))
    checked = 0
    for case in z["cases"]:
        call = json.loads(str(z[case + "__call"]))
        arr = {a[1]: z[a[2]] for a in call["args"] if a[0] == "a"}
        num, den, want = arr["b"], arr["Ax"], z[call["out"]["x"]]
        pairs = np.empty(2 * len(num), dtype=num.dtype)
        pairs[0::2], pairs[1::2] = num, den
        (tmp_path / "in.bin").write_bytes(pairs.tobytes())
        subprocess.run([str(exe), "s" if num.dtype == np.complex64 else "d", str(tmp_path / "in.bin"),
                        str(tmp_path / "out.bin"), str(len(num))], check=True)
        got = np.frombuffer((tmp_path / "out.bin").read_bytes(), dtype=num.dtype)
        u = np.uint32 if num.dtype == np.complex64 else np.uint64
        bad = np.nonzero(got.view(u) != want.view(u))[0]
        assert bad.size == 0, "%s: %d parts differ, first at %d" % (case, bad.size, bad[0])
        checked += len(num)
    assert checked == 2 * 4096
