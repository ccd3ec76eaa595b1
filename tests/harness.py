"""The plumbing every host harness shares (tests/*_host_harness.cpp and the *_cases.py module that writes its case file, runs it and
reads the results): the one g++ recipe for the stand-alone programs and the one for the two shared objects, the runner, a reader of
result files, a writer of arrays, and the bit-for-bit comparison of a result dictionary.  The C++ side of the same plumbing is
tests/harness_io.h and tests/harness_mesh.h."""
from __future__ import annotations

import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "par_raytracer_amd", "csrc")
SHIM = os.path.join(ROOT, "tests", "hip_shim")


def _compile(cmd):
    build = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert build.returncode == 0, build.stdout.decode()
    return cmd[-1]


def build(source, directory, name, *, sanitize=False, bvh8=False, sources=(), flags=()):
    """tests/<source> (and csrc/<each of sources>) as the stand-alone program <directory>/<name>, a program with its own main;
    returns its path."""
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-pthread", "-I" + SHIM, "-I" + CSRC]
    if bvh8:
        cmd += ["-DPRT_BVH8"]
    if sanitize:
        # the sanitizer runtimes are linked statically: the program then starts whatever else the environment loads ahead of it
        cmd += ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]
    cmd += list(flags) + [os.path.join(ROOT, "tests", source)] + [os.path.join(CSRC, s) for s in sources]
    return _compile(cmd + ["-o", os.path.join(str(directory), name)])


def build_shared(source, directory, name):
    """tests/<source>, which includes the CPU oracle, as the shared object <directory>/<name>; returns its path."""
    return _compile(["g++", "-O2", "-std=c++14", "-fPIC", "-shared", "-ffp-contract=off", "-fno-strict-aliasing", "-pthread",
                     "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", source), "-o", os.path.join(str(directory), name)])


def run(exe, *args, timeout=600):
    """The program's output (stdout and stderr together); a non-zero exit status fails with the output's tail."""
    done = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
    out = done.stdout.decode()
    assert done.returncode == 0, out[-4000:]
    return out


def case_files(directory, cases, results):
    return os.path.join(str(directory), cases), os.path.join(str(directory), results)


def put(f, *pairs):
    """Writes (array, dtype), (array, dtype), ... to the open file, each converted to its dtype and made contiguous."""
    for a, dt in pairs:
        f.write(np.ascontiguousarray(a, dt).tobytes())


class Reader:
    """A result file's bytes, consumed front to back."""

    def __init__(self, blob):
        self.blob, self.at = blob, 0

    @classmethod
    def of_file(cls, path):
        with open(path, "rb") as f:
            return cls(f.read())

    def take(self, count, dtype, shape=None):
        count = int(count)
        assert self.at + count * np.dtype(dtype).itemsize <= len(self.blob), "the results end %d bytes early" % (
            self.at + count * np.dtype(dtype).itemsize - len(self.blob))
        a = np.frombuffer(self.blob, dtype, count, self.at).copy()
        self.at += a.nbytes
        return a if shape is None else a.reshape(shape)

    def unpack(self, fmt):
        assert self.at + struct.calcsize(fmt) <= len(self.blob), "the results end inside a header"
        out = struct.unpack_from(fmt, self.blob, self.at)
        self.at += struct.calcsize(fmt)
        return out

    def done(self):
        assert self.at == len(self.blob), "%d bytes of the results were not read" % (len(self.blob) - self.at)


def assert_same_bits(got, expect, what, fields):
    """Every field of `got` ({field: numpy array}) equals `expect` bit for bit: equal shape, equal item size, equal bytes."""
    for k in fields:
        g, e = np.ascontiguousarray(got[k]), np.ascontiguousarray(expect[k])
        assert g.shape == e.shape and g.dtype.itemsize == e.dtype.itemsize, (what, k, g.shape, e.shape, g.dtype, e.dtype)
        rows = max(len(e), 1) if e.ndim else 1
        bad = np.nonzero((g.reshape(rows, -1).view(np.uint8) != e.reshape(rows, -1).view(np.uint8)).any(1))[0]
        assert bad.size == 0, "%s: field %s differs on %d of %d rows, first %d: got %r, expected %r" % (
            what, k, bad.size, rows, bad[0], g.reshape(rows, -1)[bad[0]].tolist(), e.reshape(rows, -1)[bad[0]].tolist())


def to_numpy(res, as_uint32=()):
    """A query's result dictionary with torch tensors -> numpy arrays, the fields of as_uint32 viewed as uint32; what is no
    tensor (the counters, the info) passes through."""
    out = {}
    for k, v in res.items():
        a = v.cpu().numpy() if hasattr(v, "cpu") else v
        out[k] = a.view(np.uint32) if k in as_uint32 else a
    return out
