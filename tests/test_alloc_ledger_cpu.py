"""The allocation ledger of a graph handle (numbskull_amd/csrc/nsk_alloc.h) is plain C++ without a HIP call: a
stand-alone program feeds it fake pointers and asserts the totals, built with the host compiler under AddressSanitizer
and UndefinedBehaviorSanitizer (-fno-sanitize-recover: any report ends the program with a failure).  A clean exit is
the pass.  The program stubs the rollback's "free" (the library's is hipFree)."""

import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "numbskull_amd", "csrc")
SANITIZE = "-fsanitize=address,undefined"

PROGRAM = r"""
#undef NDEBUG
#include <cassert>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "nsk_alloc.h"

static void *fake(uintptr_t x) { return (void *)x; }
static std::vector<void *> freed;                   // the allocations the rollback handed to its "free"
static void stub_free(void *raw) { freed.push_back(raw); }

int main() {
    NskLedger L;
    assert(L.total == 0 && L.entries.empty());
    // add and remove
    L.add(fake(0x1000), fake(0x1000), 64);
    L.add(fake(0x2000), fake(0x2000), 1);
    assert(L.total == 65 && L.entries.size() == 2);
    assert(L.remove(fake(0x1000)) == fake(0x1000));
    assert(L.total == 1 && L.entries.size() == 1 && L.entries[0].ptr == fake(0x2000));
    // an aligned alias resolves to its allocation; the allocation itself was never handed out
    L.add(fake(0x400000), fake(0x3ff010), 1 << 20);
    assert(L.total == 1 + (1 << 20));
    assert(L.remove(fake(0x3ff010)) == nullptr && L.total == 1 + (1 << 20));
    assert(L.remove(fake(0x400000)) == fake(0x3ff010) && L.total == 1);
    // unknown pointers, null, a second removal
    assert(L.remove(nullptr) == nullptr && L.remove(fake(0x9999)) == nullptr && L.remove(fake(0x1000)) == nullptr);
    assert(L.total == 1 && L.entries.size() == 1);
    // a rollback frees exactly what was added since its construction, newest first, the allocation not the alias
    L.add(fake(0x5000), fake(0x5000), 10);
    {
        NskRollback rb(L, stub_free);
        L.add(fake(0x6000), fake(0x6000), 100);
        L.add(fake(0x800000), fake(0x7ff000), 1000);
        L.add(fake(0x9000), fake(0x9000), 10000);
        assert(L.remove(fake(0x6000)) == fake(0x6000));       // one of its OWN freed by hand inside the scope: not freed twice
        assert(L.total == 1 + 10 + 1000 + 10000);
    }
    assert(freed.size() == 2 && freed[0] == fake(0x9000) && freed[1] == fake(0x7ff000));
    assert(L.total == 11 && L.entries.size() == 2);
    // ... and none after commit(), whatever went before it was freed afterwards; an empty scope frees nothing
    freed.clear();
    {
        NskRollback rb(L, stub_free);
        L.add(fake(0xb000), fake(0xb000), 5);
        L.add(fake(0xc000), fake(0xc000), 6);
        rb.commit();
        assert(L.remove(fake(0x5000)) == fake(0x5000));       // (the regrow sites: the old array goes after commit())
    }
    { NskRollback rb(L, stub_free); }
    assert(freed.empty() && L.total == 12 && L.entries.size() == 3);
    // two scopes, the inner one committed: the outer one still takes back everything since ITS construction
    {
        NskRollback outer(L, stub_free);
        L.add(fake(0xd000), fake(0xd000), 8);
        { NskRollback inner(L, stub_free); L.add(fake(0xe000), fake(0xe000), 9); inner.commit(); }
        assert(L.total == 29);
    }
    assert(freed.size() == 2 && freed[0] == fake(0xe000) && freed[1] == fake(0xd000) && L.total == 12);
    // everything removed: the total is 0
    std::vector<void *> left;
    for (const NskLedger::Entry &e : L.entries) left.push_back(e.ptr);
    assert(left.size() == 3 && left[0] == fake(0x2000));          // oldest first
    for (void *p : left) assert(L.remove(p) == p);
    assert(L.total == 0 && L.entries.empty());
    std::puts("ledger ok");
    return 0;
}
"""


def _compiler():
    """(command prefix, sanitizer flags): the host compiler, or hipcc compiling for the host only"""
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return [shutil.which(cxx)], [SANITIZE, "-fno-sanitize-recover=all"]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        return [hipcc, "-x", "c++"], ["-Xarch_host", SANITIZE, "-Xarch_host", "-fno-sanitize-recover=all"]
    return None, None


def test_ledger_and_rollback_under_sanitizers(tmp_path):
    cxx, san = _compiler()
    if cxx is None:
        pytest.skip("no C++ compiler on this machine")
    src, exe = tmp_path / "ledger_main.cpp", tmp_path / "ledger_main"
    src.write_text(PROGRAM)
    cmd = cxx + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + san + ["-I", CSRC, str(src), "-o", str(exe)]
    build = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if build.returncode != 0:       # (a compiler without these switches)
        build = subprocess.run(cmd, capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert "ledger ok" in run.stdout
