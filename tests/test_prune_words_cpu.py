"""The word-wise run / piece arithmetic of prune_slabs_kernel (csrc/glhip_prune_words.h) against the block-by-block walk it replaces
for gap length 1 (csrc/glhip_autosort.h): a piece starts at a kept block whose predecessor is not kept (a run) or at a kept block that
is a multiple of PB (the piece grid), and ends where the next one starts or behind the last kept block before a run.  The header is
plain C++; a small program around it plays the kernel's 256 threads (each counts and emits the pieces of its own words, numbered by
a prefix sum) and is compared with a serial Python walk: run count, every interval slot, the zero fill.  Inputs: random bit sets,
all-kept and none-kept ones, runs that cross word boundaries, several PB, slot counts S smaller than the number of pieces.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")
C = 256      # columns per block

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "glhip_prune_words.h"
// stdin: nT M PB S, then the words in hex; stdout: runs, pieces, then the 2 S slot values
int main() {
    int nT, M, PB, S;
    if (std::scanf("%d %d %d %d", &nT, &M, &PB, &S) != 4) return 1;
    const int nW = (nT + 63) / 64, T = 256;
    std::vector<unsigned long long> mask(nW);
    for (int w = 0; w < nW; ++w)
        if (std::scanf("%llx", &mask[w]) != 1) return 1;
    std::vector<int32_t> slots(2 * S, -7);
    const int wpt = (nW + T - 1) / T;
    std::vector<int> base(T + 1, 0);
    int runs = 0;
    for (int tid = 0; tid < T; ++tid) {
        const int w0 = std::min(nW, tid * wpt), w1 = std::min(nW, w0 + wpt);
        int r, p;
        glhip::prune_count_words(mask.data(), w0, w1, PB, r, p);
        runs += r;
        base[tid + 1] = base[tid] + p;
    }
    for (int tid = T - 1; tid >= 0; --tid) {      // (any order: the threads write disjoint slots)
        const int w0 = std::min(nW, tid * wpt), w1 = std::min(nW, w0 + wpt);
        glhip::prune_emit_words(mask.data(), w0, w1, base[tid], PB, S, 256, M, slots.data());
    }
    const int n = std::min(base[T], S);
    if (n > 0) glhip::prune_emit_last(mask.data(), nW, n, 256, M, slots.data());
    for (int q = n; q < S; ++q) slots[2 * q] = slots[2 * q + 1] = 0;
    std::printf("%d %d\n", runs, base[T]);
    for (int q = 0; q < 2 * S; ++q) std::printf("%d\n", slots[q]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def words_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("prune_words")
    src = d / "words.cpp"
    src.write_text(PROGRAM)
    exe = d / "words"
    subprocess.run([cxx, "-std=c++17", "-O1", "-I", HEADER_DIR, str(src), "-o", str(exe)], check=True)
    return str(exe)


def _words(exe, kept, M, PB, S):
    nT = len(kept)
    nW = (nT + 63) // 64
    bits = np.zeros(nW * 64, np.uint64)
    bits[:nT] = kept
    words = (bits.reshape(nW, 64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    text = f"{nT} {M} {PB} {S}\n" + "\n".join(f"{int(v):x}" for v in words) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    return int(out[0]), int(out[1]), np.array(out[2:], np.int64).reshape(S, 2)


def _walk(kept, M, PB, S):
    """prune_slabs_kernel's walk(1, emit), block by block"""
    slots = np.zeros((S, 2), np.int64)
    prev, runs, pieces = -1, 0, 0
    for t in np.flatnonzero(kept):
        run = prev < 0 or t - prev - 1 >= 1
        if run or t % PB == 0:
            if pieces < S:
                slots[pieces, 0] = t * C
                if pieces > 0:
                    slots[pieces - 1, 1] = min(M, ((prev + 1) if run else t) * C)
            pieces += 1
        runs += run
        prev = t
    n = min(pieces, S)
    if n > 0:
        slots[n - 1, 1] = min(M, (prev + 1) * C)
    return runs, pieces, slots


def _cases():
    g = np.random.default_rng(7)
    for nT in (1, 63, 64, 65, 200, 3907, 20000):
        yield np.ones(nT, bool)
        yield np.zeros(nT, bool)
        for p in (0.02, 0.5, 0.97):
            yield g.random(nT) < p
        k = np.zeros(nT, bool)      # long runs and long gaps
        for a in g.integers(0, nT, 12):
            k[a:a + int(g.integers(1, 400))] = True
        yield k
    k = np.zeros(320, bool)       # runs across word boundaries: one that ends on bit 63, one that starts on bit 0, one over three words
    k[60:64] = True
    k[128:131] = True
    k[180:300] = True
    yield k
    k = np.zeros(256, bool)       # a lone block on bit 63 and its neighbour on bit 0 of the next word; the last block of all
    k[63] = True
    k[64] = True
    k[191] = True
    k[255] = True
    yield k


def test_words_match_the_walk(words_exe):
    n = 0
    for kept in _cases():
        nT = len(kept)
        M = nT * C - 219 if nT > 1 else 37      # the last block is partial
        for PB in (64, 65, 100, 1000):
            full = int(_walk(kept, M, PB, 10**6)[1])
            for S in sorted({max(full, 1) + 3, max(full // 2, 1)}):      # room for every piece, and fewer slots than pieces
                runs, pieces, slots = _words(words_exe, kept, M, PB, S)
                want_runs, want_pieces, want = _walk(kept, M, PB, S)
                assert (runs, pieces) == (want_runs, want_pieces), (nT, PB, S)
                assert np.array_equal(slots, want), (nT, PB, S)
                n += 1
    assert n >= 200
