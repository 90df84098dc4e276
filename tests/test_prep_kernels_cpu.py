"""The host side of the cheaper preparation kernels of the pruned p = 2 call (csrc/glhip_prune.hip), on the plain-C++ headers.

Gap closing from the bit set (csrc/glhip_prune_words.h).  A slab with more than kPruneRuns runs of kept blocks closes its smallest gaps:
g is the smallest gap length that leaves at most kPruneRuns runs, a run starts at the first kept block or at one with at least g blocks
that are not kept in front of it, grid cuts stay on the kept bits at multiples of PB, and a run's predecessor piece ends behind the last
kept block.  prune_slabs_kernel takes the gap lengths, g, the counts and the pieces from the 64-bit words; a small program plays its 256
threads (each on its own words, numbered by prefix sums, g by the serial rule and by the kernel's bisection in rounds of 256 gaps) and
is compared with a serial Python walk(g, emit): g, the run count, the piece count, every slot, the zero fill.

The balancing pass (csrc/glhip_balance.h).  The levels above the last leave out the steps of their last merge after the first
(balance_step_runs); the program plays the kernel's 1024 threads with and without those steps, and both orders must equal the model's
(tools/prune_model.py: balanced_order): random blocks for D = 1, 2, 3, blocks with many ties, the special values of
tests/test_balanced_order_cpu.py (NaN, infinities, signed zeros, duplicates) and identical points, which come out in incoming order.

Both programs are built with the address and undefined-behaviour sanitizers where the host compiler has them.
"""

import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import prune_model as pm  # noqa: E402

C = 256          # columns per block
RUNS = 160       # kPruneRuns
assert pm.RUNS == RUNS and pm.BLOCK == C


def _build(tmp_path_factory, name, program):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp(name)
    src = d / f"{name}.cpp"
    src.write_text(program)
    exe = d / name
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", HEADER_DIR, str(src), "-o", str(exe)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:      # a compiler without the sanitizer runtimes: the comparison is the same
        subprocess.run(base, check=True)
    return str(exe)


# ---- gap closing from the words ------------------------------------------------------------------------------------------------------

GAP_PROGRAM = r"""
#include <algorithm>
#include <cstdio>
#include <vector>
#include "glhip_prune_words.h"
// stdin: nT M PB S RUNS, then the words in hex; stdout: g, runs for g = 1, runs for g, pieces, then the 2 S slot values
int main() {
    int nT, M, PB, S, RUNS;
    if (std::scanf("%d %d %d %d %d", &nT, &M, &PB, &S, &RUNS) != 5) return 1;
    const int nW = (nT + 63) / 64, T = 256;
    std::vector<unsigned long long> mask(nW);
    for (int w = 0; w < nW; ++w)
        if (std::scanf("%llx", &mask[w]) != 1) return 1;
    std::vector<int32_t> slots(2 * S, -7);
    const int wpt = (nW + T - 1) / T;
    auto w0_of = [&](int tid) { return std::min(nW, tid * wpt); };
    auto w1_of = [&](int tid) { return std::min(nW, w0_of(tid) + wpt); };
    std::vector<int> run0(T + 1, 0), base(T + 1, 0);
    for (int tid = 0; tid < T; ++tid) {
        int r, p;
        glhip::prune_count_words(mask.data(), w0_of(tid), w1_of(tid), PB, r, p);
        run0[tid + 1] = run0[tid] + r;
    }
    const int runs1 = run0[T];
    int g = 1;
    if (runs1 > RUNS) {
        const int n = runs1 - 1, guard = 8;
        std::vector<int32_t> gaps(n + guard, -7);
        for (int tid = T - 1; tid >= 0; --tid)      // (any order: the threads write disjoint entries)
            glhip::prune_gap_lengths(mask.data(), w0_of(tid), w1_of(tid), run0[tid], n, gaps.data());
        for (int q = 0; q < n; ++q)
            if (gaps[q] < 1) return 3;              // every gap written, none empty
        for (int q = n; q < n + guard; ++q)
            if (gaps[q] != -7) return 4;            // nothing behind the list
        {   // a list that is too short is not overrun
            std::vector<int32_t> few(n / 2 + guard, -7);
            for (int tid = 0; tid < T; ++tid) glhip::prune_gap_lengths(mask.data(), w0_of(tid), w1_of(tid), run0[tid], n / 2, few.data());
            for (int q = 0; q < n / 2 + guard; ++q)
                if (few[q] != (q < n / 2 ? gaps[q] : -7)) return 5;
        }
        g = glhip::prune_gap_select(gaps.data(), n, RUNS, nT);
        int lo = 0, hi = nT;                        // the kernel's form: one count per step and round of 256 gaps
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            int c = 0;
            for (int q0 = 0; q0 < n; q0 += T)
                for (int tid = 0; tid < T; ++tid) c += q0 + tid < n && gaps[q0 + tid] >= mid;
            if (1 + c > RUNS) lo = mid; else hi = mid;
        }
        if (hi != g) return 6;
    }
    int runs = 0;
    for (int tid = 0; tid < T; ++tid) {
        int r, p;
        glhip::prune_count_words(mask.data(), w0_of(tid), w1_of(tid), PB, r, p, g);
        runs += r;
        base[tid + 1] = base[tid] + p;
    }
    for (int tid = T - 1; tid >= 0; --tid)
        glhip::prune_emit_words(mask.data(), w0_of(tid), w1_of(tid), base[tid], PB, S, 256, M, slots.data(), g);
    const int n = std::min(base[T], S);
    if (n > 0) glhip::prune_emit_last(mask.data(), nW, n, 256, M, slots.data());
    for (int q = n; q < S; ++q) slots[2 * q] = slots[2 * q + 1] = 0;
    std::printf("%d %d %d %d\n", g, runs1, runs, base[T]);
    for (int q = 0; q < 2 * S; ++q) std::printf("%d\n", slots[q]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def gap_exe(tmp_path_factory):
    return _build(tmp_path_factory, "gap_words", GAP_PROGRAM)


def _words(exe, kept, M, PB, S):
    nT = len(kept)
    nW = (nT + 63) // 64
    bits = np.zeros(nW * 64, np.uint64)
    bits[:nT] = kept
    words = (bits.reshape(nW, 64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)
    text = f"{nT} {M} {PB} {S} {RUNS}\n" + "\n".join(f"{int(v):x}" for v in words) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split()
    return tuple(int(v) for v in out[:4]), np.array(out[4:], np.int64).reshape(S, 2)


def _walk(kept, M, PB, S, g):
    """prune_slabs_kernel's walk(g, emit), block by block"""
    slots = np.zeros((S, 2), np.int64)
    prev, runs, pieces = -1, 0, 0
    for t in np.flatnonzero(kept):
        run = prev < 0 or t - prev - 1 >= g
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


def _runs(kept, g):
    idx = np.flatnonzero(kept)
    return 0 if len(idx) == 0 else 1 + int((np.diff(idx) - 1 >= g).sum())


def _choose_g(kept):
    """the kernel's rule: g = 1 unless that leaves more than RUNS runs; then the smallest gap length that does not (walk(nT) has one run)"""
    if _runs(kept, 1) <= RUNS:
        return 1
    lo, hi = 1, len(kept)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if _runs(kept, mid) > RUNS:
            lo = mid
        else:
            hi = mid
    return hi


def _from_gaps(gaps, lens, first=0):
    """a bit set: `first` blocks that are not kept, then runs of lens[i] kept blocks with gaps[i] blocks between them"""
    out = [np.zeros(first, bool)]
    for i, n in enumerate(lens):
        out.append(np.ones(n, bool))
        if i < len(gaps):
            out.append(np.zeros(gaps[i], bool))
    return np.concatenate(out)


def _gap_cases():
    g = np.random.default_rng(11)
    for nT in (1, 63, 64, 65, 200, 3907, 20000):
        yield np.ones(nT, bool)
        for p in (0.03, 0.2, 0.5, 0.9):
            yield g.random(nT) < p
    for runs in (161, 162, 200, 500, 1999, 2000):      # 161 to 2000 runs, gaps of 1 to 30 blocks, runs of 1 to 5
        yield _from_gaps(g.integers(1, 31, runs - 1), g.integers(1, 6, runs), first=int(g.integers(0, 70)))
    # many gaps of one length at the run limit: 100 long gaps, 300 of 3 blocks (g = 4 closes all 300 of them: 101 runs, not 160) ...
    gaps = np.concatenate([np.full(100, 9), np.full(300, 3), np.full(50, 1)])
    yield _from_gaps(g.permutation(gaps), g.integers(1, 4, len(gaps) + 1))
    # ... exactly RUNS - 1 gaps above the rest (g = 3: they alone stay open), and exactly RUNS of them (g = 8: one too many stays at 7)
    gaps = np.concatenate([np.full(RUNS - 1, 7), np.full(400, 2)])
    yield _from_gaps(g.permutation(gaps), g.integers(1, 4, len(gaps) + 1))
    gaps = np.concatenate([np.full(RUNS, 7), np.full(400, 2)])
    yield _from_gaps(g.permutation(gaps), g.integers(1, 4, len(gaps) + 1))
    yield _from_gaps(np.full(400, 5), np.ones(401, int))      # every gap alike: g = 6 leaves one run
    # gaps across word and thread boundaries (20000 blocks: 313 words, 2 words per thread): lone kept blocks on bits 63 and 0, gaps of
    # 63 to 130 blocks that span whole words that are not kept, among 300 short gaps
    k = np.zeros(20000, bool)
    k[63::128] = True
    k[64::256] = True
    k[5000:5900:3] = True
    yield k
    k = np.zeros(20000, bool)
    k[0:19000:127] = True
    k[19000:19999:2] = True
    yield k
    # a multiple of PB inside a closed gap (PB = 100: blocks 100, 200, ... are not kept) and on a kept block inside a closed run
    k = np.zeros(3907, bool)
    k[1:3900:4] = True                  # 975 runs with gaps of 3
    k[99:3900:100] = True               # ... every multiple of 100 inside a gap that closes
    k[2000:2010] = False                # two long gaps stay
    k[3000:3050] = False
    yield k
    k = np.zeros(3907, bool)
    k[0:3900:4] = True                  # the multiples of 64, 100 and 1000 are kept blocks, in the middle of runs of closed gaps
    k[1200:1300] = False
    yield k


def test_gap_words_match_the_walk(gap_exe):
    n = over = 0
    seen_g = set()
    for kept in _gap_cases():
        nT = len(kept)
        M = nT * C - 219 if nT > 1 else 37      # the last block is partial
        g = _choose_g(kept)
        for PB in (64, 65, 100, 1000):
            full = _walk(kept, M, PB, 10**6, g)[1]
            for S in sorted({max(full, 1) + 3, max(full // 2, 1)}):      # room for every piece, and fewer slots than pieces
                (got_g, runs1, runs, pieces), slots = _words(gap_exe, kept, M, PB, S)
                want_runs, want_pieces, want = _walk(kept, M, PB, S, g)
                assert got_g == g and runs1 == _runs(kept, 1), (nT, PB, S)
                assert (runs, pieces) == (want_runs, want_pieces) and runs <= max(RUNS, 1), (nT, PB, S, g)
                assert np.array_equal(slots, want), (nT, PB, S, g)
                n += 1
        over += g > 1
        seen_g.add(g)
    print(f"{n} comparisons, {over} bit sets over the run limit, gap lengths {sorted(seen_g)}")
    assert n >= 300 and over >= 12 and len(seen_g) >= 6


def test_gap_length_rule():
    """the serial rule of the header against its definition: one more than the RUNS-th longest gap"""
    g = np.random.default_rng(12)
    for _ in range(50):
        gaps = g.integers(1, 40, int(g.integers(RUNS, 1500)))
        kept = _from_gaps(gaps, np.ones(len(gaps) + 1, int))
        assert _choose_g(kept) == np.sort(gaps)[::-1][RUNS - 1] + 1


# ---- the balancing pass: partition the upper levels, sort the last --------------------------------------------------------------------

BLOCK = 1024

BALANCE_PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
#include "glhip_balance.h"
// stdin: full (1: every step of five sorts, the network as it was; 0: the steps of balance_step_runs), D, then 1024 x D bit patterns of
// a block's points in their incoming order -> the number of steps run, then the incoming position of the point at every place
using namespace glhip;
static float from_bits(unsigned b) { float f; std::memcpy(&f, &b, 4); return f; }
int main() {
    const int B = 1024;
    int full, D;
    if (std::scanf("%d %d", &full, &D) != 2 || D < 1 || D > 3) return 1;
    std::vector<float> pts(3 * B, 0.f);
    for (int i = 0; i < B; ++i)
        for (int d = 0; d < D; ++d) {
            unsigned b;
            if (std::scanf("%x", &b) != 1) return 1;
            pts[d * B + i] = from_bits(b);
        }
    std::vector<int> p(B);
    for (int i = 0; i < B; ++i) p[i] = i;
    std::vector<unsigned long long> v(B), o(B);
    int steps = 0;
    for (int seg = B; seg >= 64; seg >>= 1) {
        for (int s0 = 0; s0 < B; s0 += seg) {
            float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int i = s0; i < s0 + seg; ++i)
                for (int d = 0; d < D; ++d) balance_extent_add(pts[d * B + p[i]], lo[d], hi[d]);
            const int axis = balance_axis(lo, hi, 3);
            for (int i = s0; i < s0 + seg; ++i) v[i] = balance_word(balance_key(pts[axis * B + p[i]]), (unsigned)p[i]);
        }
        for (int k = 2; k <= seg; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                if (!full && !balance_step_runs(j, k, seg, 64)) break;
                for (int i = 0; i < B; ++i) o[i] = v[i ^ j];
                for (int i = 0; i < B; ++i) v[i] = (balance_keeps_min(i, j, k, seg) == (o[i] < v[i])) ? o[i] : v[i];
                ++steps;
            }
        for (int i = 0; i < B; ++i) p[i] = (int)(unsigned)v[i];
    }
    std::printf("%d\n", steps);
    for (int i = 0; i < B; ++i) std::printf("%d\n", p[i]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def balance_exe(tmp_path_factory):
    return _build(tmp_path_factory, "balance_partition", BALANCE_PROGRAM)


def _cloud(n, D, seed):
    return np.random.default_rng(seed).random((n, D), dtype=np.float32)


def _special_blocks():
    """the special-value cloud of tests/test_balanced_order_cpu.py, block by block: NaN of both signs, infinities, signed zeros,
    duplicated points, a block of identical points, a cell's worth of points without one finite coordinate"""
    g = np.random.default_rng(5)
    z = g.random((3 * BLOCK + 77, 3), dtype=np.float32)
    z[g.integers(0, BLOCK, 40), g.integers(0, 3, 40)] = np.nan
    z[7, 0] = -np.float32(np.nan)
    z[g.integers(0, BLOCK, 10), g.integers(0, 3, 10)] = np.inf
    z[g.integers(0, BLOCK, 10), g.integers(0, 3, 10)] = -np.inf
    z[100:110, 1] = 0.0
    z[110:120, 1] = -0.0
    z[200:600] = z[200]
    z[BLOCK:2 * BLOCK] = np.float32(0.25)
    z[2 * BLOCK:2 * BLOCK + 64] = np.nan
    return [z[:BLOCK], z[BLOCK:2 * BLOCK], z[2 * BLOCK:3 * BLOCK]]


def _order(exe, block_pts, full):
    D = block_pts.shape[1]
    bits = "\n".join(f"{int(b):x}" for b in np.ascontiguousarray(block_pts, np.float32).view(np.uint32).ravel())
    out = subprocess.run([exe], input=f"{int(full)} {D}\n{bits}\n", capture_output=True, text=True, check=True).stdout.split()
    return int(out[0]), np.array(out[1:], np.int64)


def test_balance_partition_matches_the_model_and_the_network(balance_exe):
    blocks = [_cloud(BLOCK, D, 70 + 10 * D + s) for D in (1, 2, 3) for s in range(3)]
    blocks.append((np.round(_cloud(BLOCK, 3, 90) * 8) / 8).astype(np.float32))      # many ties on every axis: the position decides
    blocks.append((np.round(_cloud(BLOCK, 2, 91) * 4) / 4).astype(np.float32))
    blocks.append((np.round(_cloud(BLOCK, 1, 92) * 2) / 2).astype(np.float32))
    blocks += _special_blocks()
    for pts in blocks:
        want = pm.balanced_order(pts, np.arange(BLOCK))
        steps_full, net = _order(balance_exe, pts, True)
        steps, got = _order(balance_exe, pts, False)
        assert (steps_full, steps) == (185, 155)
        assert np.array_equal(np.sort(got), np.arange(BLOCK))
        assert np.array_equal(net, want) and np.array_equal(got, want)
    same = np.full((BLOCK, 3), 0.25, np.float32)                                     # identical points: the incoming order
    assert np.array_equal(_order(balance_exe, same, False)[1], np.arange(BLOCK))
