"""The sorted candidate lists of the top-k arg-reduction (csrc/glhip_topk_list.h) on the host: a small program feeds streams of
(u, index) through ``topk_push`` (indices ascending, strict compare), ``topk_insert_lex`` (any order) and ``topk_merge`` for the
capacities 1, 4, 8 and 16, sorts the same candidates with ``std::stable_sort`` under the lexicographic rule (u descending, index
ascending; -inf and NaN never enter; empty entries are (-inf, -1)) and prints both.  The test compares them bit for bit, and against
its own Python sort.

Streams: random values, runs of exact ties, strictly increasing and strictly decreasing u, -inf, +inf and NaN among the values, fewer
items than the capacity, none at all.  The program is built with the address and undefined-behaviour sanitizers where the host
compiler has them.
"""

import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")
CAPS = (1, 4, 8, 16)

PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "glhip_topk_list.h"
struct Item { float u; int i; };
static float from_bits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
static uint32_t bits(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static bool read_items(std::vector<Item>& v, int n) {
    v.resize(n);
    for (auto& it : v) {
        unsigned b;
        if (std::scanf("%x %d", &b, &it.i) != 2) return false;
        it.u = from_bits(b);
    }
    return true;
}
template <int CAP> static void print_list(const char* tag, const float (&lu)[CAP], const int (&li)[CAP]) {
    std::printf("%s", tag);
    for (int r = 0; r < CAP; ++r) std::printf(" %08x %d", bits(lu[r]), li[r]);
    std::printf("\n");
}
// the reference: admissible candidates (u > -inf, not NaN) under (u descending, index ascending), the first CAP, padded with (-inf, -1)
template <int CAP> static void reference(std::vector<Item> v) {
    v.erase(std::remove_if(v.begin(), v.end(), [](const Item& a) { return !(a.u > -__builtin_inff()); }), v.end());
    std::stable_sort(v.begin(), v.end(), [](const Item& a, const Item& b) { return glhip::topk_beats(a.u, a.i, b.u, b.i); });
    float lu[CAP];
    int li[CAP];
    glhip::topk_clear<CAP>(lu, li);
    for (int r = 0; r < CAP && r < (int)v.size(); ++r) { lu[r] = v[r].u; li[r] = v[r].i; }
    print_list<CAP>("R", lu, li);
}
// stdin per case: mode ('P' push: one stream, indices ascending | 'M' merge: two streams in any order), na, nb, the items
template <int CAP> static bool run(char mode, int na, int nb) {
    std::vector<Item> a, b;
    if (!read_items(a, na) || !read_items(b, nb)) return false;
    float lu[CAP], ou[CAP];
    int li[CAP], oi[CAP];
    glhip::topk_clear<CAP>(lu, li);
    glhip::topk_clear<CAP>(ou, oi);
    if (mode == 'P') {
        for (const Item& it : a) glhip::topk_push<CAP>(lu, li, it.u, it.i);
    } else {
        for (const Item& it : a) glhip::topk_insert_lex<CAP>(lu, li, it.u, it.i);
        for (const Item& it : b) glhip::topk_insert_lex<CAP>(ou, oi, it.u, it.i);
        glhip::topk_merge<CAP>(lu, li, ou, oi);
    }
    print_list<CAP>("L", lu, li);
    a.insert(a.end(), b.begin(), b.end());
    reference<CAP>(a);
    return true;
}
int main() {
    char mode;
    int cap, na, nb;
    while (std::scanf(" %c %d %d %d", &mode, &cap, &na, &nb) == 4) {
        bool ok = false;
        switch (cap) {
            case 1: ok = run<1>(mode, na, nb); break;
            case 4: ok = run<4>(mode, na, nb); break;
            case 8: ok = run<8>(mode, na, nb); break;
            case 16: ok = run<16>(mode, na, nb); break;
        }
        if (!ok) return 1;
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("topk_list")
    src = d / "topk_list.cpp"
    src.write_text(PROGRAM)
    out = d / "topk_list"
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", HEADER_DIR, str(src), "-o", str(out)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:      # a compiler without the sanitizer runtimes: the comparison is the same
        subprocess.run(base, check=True)
    return str(out)


def _bits(u):
    return struct.unpack("<I", struct.pack("<f", u))[0]


def _expected(items, cap):
    """The Python sort: admissible items by (u descending, index ascending), padded with (-inf, -1)."""
    ok = [(np.float32(u), i) for u, i in items if np.float32(u) > -np.inf]
    ok.sort(key=lambda t: (-float(t[0]), t[1]))
    ok = ok[:cap] + [(np.float32(-np.inf), -1)] * max(0, cap - len(ok))
    return [(_bits(float(u)), i) for u, i in ok]


def _streams(rng):
    """(name, values): float32 streams of every kind the docstring lists."""
    inf, nan = np.inf, np.nan
    out = [("empty", np.zeros(0, np.float32)), ("three items", rng.standard_normal(3).astype(np.float32))]
    out.append(("random", rng.standard_normal(200).astype(np.float32)))
    out.append(("ties", rng.integers(0, 4, 200).astype(np.float32)))
    out.append(("all equal", np.full(50, 1.5, np.float32)))
    out.append(("increasing", np.arange(100, dtype=np.float32)))
    out.append(("decreasing", -np.arange(100, dtype=np.float32)))
    v = rng.integers(0, 6, 200).astype(np.float32)
    v[rng.permutation(200)[:60]] = rng.choice([-inf, inf, nan], 60)
    out.append(("special values", v))
    out.append(("only -inf and NaN", rng.choice([-inf, nan], 40).astype(np.float32)))
    return out


def _run(exe, cases):
    text = []
    for mode, cap, a, b in cases:
        text.append(f"{mode} {cap} {len(a)} {len(b)}")
        text += [f"{_bits(float(u)):x} {i}" for u, i in list(a) + list(b)]
    res = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.split("\n")[:-1]
    assert len(lines) == 2 * len(cases)
    parse = lambda ln: [(int(t[0], 16), int(t[1])) for t in zip(ln.split()[1::2], ln.split()[2::2])]  # noqa: E731
    return [(parse(lines[2 * c]), parse(lines[2 * c + 1])) for c in range(len(cases))]


def _same(got, want):
    """Bit for bit: lists of (float32 bits, index)."""
    return got == want


@pytest.mark.parametrize("cap", CAPS)
def test_push_streams(exe, cap):
    rng = np.random.default_rng(cap)
    names, cases = [], []
    for name, v in _streams(rng):
        names.append(name)
        cases.append(("P", cap, list(zip(v.tolist(), range(len(v)))), []))      # indices ascend along the stream
    for name, (got, ref), (_, _, a, _) in zip(names, _run(exe, cases), cases):
        assert _same(got, ref), (name, got, ref)
        assert _same(got, _expected(a, cap)), name


@pytest.mark.parametrize("cap", CAPS)
def test_merge_streams(exe, cap):
    rng = np.random.default_rng(100 + cap)
    names, cases = [], []
    streams = _streams(rng)
    for name_a, va in streams:
        for name_b, vb in streams[::2]:
            perm = rng.permutation(len(va) + len(vb))                           # distinct indices, in no order
            a = list(zip(va.tolist(), perm[:len(va)].tolist()))
            b = list(zip(vb.tolist(), perm[len(va):].tolist()))
            names.append(f"{name_a} + {name_b}")
            cases.append(("M", cap, a, b))
    for name, (got, ref), (_, _, a, b) in zip(names, _run(exe, cases), cases):
        assert _same(got, ref), (name, got, ref)
        assert _same(got, _expected(a + b, cap)), name


def test_prefix_property(exe):
    """The list of capacity 4 is the head of the list of capacity 16 on the same stream: what makes k a prefix of any larger k."""
    rng = np.random.default_rng(7)
    v = rng.integers(0, 8, 300).astype(np.float32)
    a = list(zip(v.tolist(), range(len(v))))
    (l4, _), (l8, _), (l16, _) = _run(exe, [("P", 4, a, []), ("P", 8, a, []), ("P", 16, a, [])])
    assert l16[:4] == l4 and l16[:8] == l8
