"""Host builds of the stand-alone check programs under tests/native/ (each has its own main and
includes headers of csrc/): one recipe for the plain build and for the one under ASan + UBSan, and one
way to run both and demand the same answer.  Nothing here is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_gxx = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def build(source, outdir, kinds=("plain", "sanitized"), sanitized_opt="-O1"):
    """tests/native/<source> compiled into outdir, once per kind: "plain" is -O2, "sanitized" is
    sanitized_opt with -fsanitize=address,undefined, where the first report ends the program.
    Returns the executables in the order of kinds."""
    exes = []
    for kind in kinds:
        flags = ["-O2"] if kind == "plain" else [sanitized_opt, "-g", "-fsanitize=address,undefined",
                                                  "-fno-sanitize-recover=all"]
        exe = str(outdir / (os.path.splitext(source)[0] + "_" + kind))
        subprocess.check_call(["g++", "-std=c++17", *flags, "-I",
                               os.path.join(ROOT, "gnark_crypto_primitives_amd", "csrc"),
                               os.path.join(ROOT, "tests", "native", source), "-o", exe])
        exes.append(exe)
    return exes


_built = {}


def build_once(source, tmp_path_factory):
    """(directory, [plain, sanitized]) of a program that several test modules drive: built for the
    first module that asks, in a directory that lasts as long as the session"""
    if source not in _built:
        d = tmp_path_factory.mktemp(os.path.splitext(source)[0])
        _built[source] = d, build(source, d)
    return _built[source]


def run_both(exes, args=(), stdin=None, out_file=None, timeout=600, check=True):
    """Every build run with the same arguments and stdin: (return code, stdout, bytes of out_file or
    None), which must be the same from all of them; with check, the return code must be 0."""
    got, errs = [], []
    for exe in exes:
        if out_file and os.path.exists(out_file):
            os.remove(out_file)
        p = subprocess.run([exe, *args], input=stdin, text=True, capture_output=True, timeout=timeout)
        blob = None
        if out_file and os.path.exists(out_file):
            with open(out_file, "rb") as f:
                blob = f.read()
        got.append((p.returncode, p.stdout, blob))
        errs.append(p.stderr[-4000:])
    assert all(g == got[0] for g in got), \
        "the plain and the sanitized build disagree: return codes %s\n%s" % ([g[0] for g in got], "\n".join(errs))
    assert got[0][0] == 0 or not check, got[0][1][-2000:] + errs[0]
    return got[0]
