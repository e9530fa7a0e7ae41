"""tests/oracle_build.py on two tiny files: the library's name follows the content of the source and of every dependency,
and a library that exists is not compiled again."""
import ctypes as C
import os

import oracle_build


def write(path, text):
    with open(path, "w") as f:
        f.write(text)


def test_the_name_follows_every_input_and_an_existing_library_is_not_rebuilt(tmp_path):
    src, dep = str(tmp_path / "answer.cpp"), str(tmp_path / "answer.hpp")
    name = "oracle_build_test_%d" % os.getpid()
    write(dep, "const int kAnswer = 41;\n")
    write(src, '#include "answer.hpp"\nextern "C" int answer() { return kAnswer; }\n')
    first = oracle_build.so_path(name, src, (dep,))
    made = []
    try:
        assert oracle_build.so_path(name, src, (dep,)) == first                  # nothing changed: the same name
        assert oracle_build.so_path(name, src) != first                          # the dependency is part of the hash
        L = oracle_build.load(name, src, (dep,))
        made.append(first)
        assert L.answer() == 41 and os.path.exists(first)
        assert not [f for f in os.listdir(os.path.dirname(first)) if f.endswith(".tmp")]
        stamp = os.stat(first).st_mtime_ns
        os.utime(first, ns=(stamp - 10 ** 9, stamp - 10 ** 9))                    # a rebuild would bring the present back
        assert oracle_build.load(name, src, (dep,)).answer() == 41
        assert os.stat(first).st_mtime_ns == stamp - 10 ** 9

        write(dep, "const int kAnswer = 42;\n")                                   # the header alone changes
        second = oracle_build.so_path(name, src, (dep,))
        assert second != first
        made.append(second)
        assert oracle_build.load(name, src, (dep,)).answer() == 42

        write(src, '#include "answer.hpp"\nextern "C" int answer() { return kAnswer + 1; }\n')
        third = oracle_build.so_path(name, src, (dep,))
        assert third not in (first, second)
        made.append(third)
        assert oracle_build.load(name, src, (dep,)).answer() == 43
        write(dep, "const int kAnswer = 41;\n")                                   # back to the first header, not to the first name
        assert oracle_build.so_path(name, src, (dep,)) not in (first, second, third)
    finally:
        for so in made:
            if os.path.exists(so):
                os.remove(so)
        if os.path.isdir(os.path.dirname(first)):
            os.rmdir(os.path.dirname(first))


def test_ptr_is_null_for_nothing():
    import numpy as np
    a = np.arange(3, dtype=np.float32)
    assert oracle_build.ptr(None) is None and oracle_build.ptr(a[:0]) is None
    assert oracle_build.ptr(a).value == a.ctypes.data and isinstance(oracle_build.ptr(a), C.c_void_p)
