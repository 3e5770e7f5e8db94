"""A NumPy stand-in for pyamg_amd.krylov's device-vector classes (a krylov.VectorSpace of float64 or complex128 host
arrays): lets the Krylov drivers' host logic (restart bookkeeping, breakdown branches, 1 x 1 systems) run without a GPU.
Handles are indices into a list of arrays; the Householder sequences and reflector storage are the base class's."""
import numpy as np

from pyamg_amd.krylov import VectorSpace


class NumpyVectors(VectorSpace):
    def __init__(self, A, M=None, dtype=np.float64):
        self.Amat = A
        self.Mfun = M
        self.n = A.shape[0]
        self.dtype = np.dtype(dtype).type
        self.real = self.dtype is np.float64
        self.store = []

    def new(self, count=None):
        self.store.append(np.zeros(self.n if count is None else count, dtype=self.dtype))
        return len(self.store) - 1

    def upload(self, host, dst=None):
        dst = self.new() if dst is None else dst
        self.store[dst][:] = np.ravel(host)
        return dst

    def download(self, src, count=None, offset=0):
        count = self.n if count is None else count
        return self.store[src][offset:offset + count].copy()

    def poke(self, dst, offset, values):
        v = np.atleast_1d(values)
        self.store[dst][offset:offset + len(v)] = v

    def peek(self, src, offset):
        v = self.store[src][offset]
        return float(v) if self.real else v

    def copy(self, dst, src, off=0):
        self.store[dst][off:] = self.store[src][off:]

    def fill(self, x, value, off=0):
        self.store[x][off:] = value

    def scale(self, out, x, c):
        self.store[out][:] = c * self.store[x]

    def axpy(self, y, a, x):
        self.store[y] += a * self.store[x]

    def xpby(self, p, beta, z):
        self.store[p][:] = beta * self.store[p] + self.store[z]

    def sub(self, out, a, b):
        self.store[out][:] = self.store[a] - self.store[b]

    def dot(self, x, y):
        if self.real:
            return float(np.dot(self.store[x], self.store[y]))
        return np.complex128(np.vdot(self.store[x], self.store[y]))

    def norm(self, x, off=0):
        return float(np.linalg.norm(self.store[x][off:]))

    def A(self, x, out):
        self.store[out][:] = self.Amat @ self.store[x]

    def AH(self, x, out):
        self.store[out][:] = self.Amat.conj().T @ self.store[x]

    def M(self, r, out):
        self.store[out][:] = self.store[r] if self.Mfun is None else self.Mfun(self.store[r])
