"""The one compile-on-first-use loader of the scalar restatements under tests/cpp/: g++ -O2 -ffp-contract=off (the
reference is x86-64 without FMA) into a temporary directory, under a name that holds the hash of everything the
library is made of, so an edit of any of it is a new file and two processes never load each other's half-written one."""
import ctypes as C
import hashlib
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "slam_mi355x.h")


def so_path(name, source, deps=()):
    """Where the library of `source` lives: the hash covers the source, the C header and every file of `deps`."""
    h = hashlib.sha1()
    for f in (source, HEADER) + tuple(deps):
        h.update(open(f, "rb").read())
    return os.path.join(tempfile.gettempdir(), "slam_%s_%d" % (name, os.getuid()), "%s_%s.so" % (name, h.hexdigest()[:16]))


def load(name, source, deps=()):
    """The CDLL of `source` (`deps`: the headers it includes besides the C header), compiled unless it exists already."""
    so = so_path(name, source, deps)
    if not os.path.exists(so):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        tmp = so + ".%d.tmp" % os.getpid()
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I", os.path.join(ROOT, "include"), source, "-o", tmp])
        os.replace(tmp, so)
    return C.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.size else None
