"""The cursor of the list-driven sweep (csrc/glhip_list_cursor.h) on the host: a small program plays one wavefront's walk — interval
slots split, split + ns, ... of a slab, batches of up to 64 groups, the kept groups popped in ascending order from the batch's keep
set, the ring's three prefetches past the last kept group — and prints every group it consumes and every group index it forms an
address from.  Against a serial Python walk: the consumed groups are exactly the kept groups of the split's intervals, in order; every
batch lies inside one interval; every address index lies in [0, n_groups - 1].

Cases: whole blocks of 256 columns as the prune kernels emit them, a cloud whose last group is partial and whose last piece is shorter
than a batch, pieces of exactly one and two batches and of one block more, empty slots between and behind the pieces, one to five column splits, keep sets
that are empty, full and random.  The program is built with the address and undefined-behaviour sanitizers where the host compiler
has them.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "geomloss_amd", "csrc")

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "glhip_list_cursor.h"
// stdin: n_slots ns n_groups, the 2 n_slots slot values, then n_groups keep bits; stdout per split: "S <split>", per batch
// "B <g0> <ng>", per consumed group "C <g>", per address index "A <g>"
int main() {
    int S, ns, nG;
    if (std::scanf("%d %d %d", &S, &ns, &nG) != 3) return 1;
    std::vector<int32_t> slots(2 * S);
    for (auto& v : slots)
        if (std::scanf("%d", &v) != 1) return 1;
    std::vector<int> kept(nG);
    for (auto& v : kept)
        if (std::scanf("%d", &v) != 1) return 1;
    const int glast = nG - 1;
    for (int split = 0; split < ns; ++split) {
        std::printf("S %d\n", split);
        glhip::ListCursor cur = glhip::list_begin(slots.data(), 0, S, split, ns);
        while (cur.q < S) {
            int g0, ng;
            cur = glhip::list_next(slots.data(), S, ns, cur, g0, ng);
            std::printf("B %d %d\n", g0, ng);
            unsigned long long keep = 0;
            for (int l = 0; l < 64; ++l) {      // lane l tests the record of group clamp(g0 + l)
                const int g = glhip::list_clamp(g0 + l, glast);
                std::printf("A %d\n", g);
                if (kept[g]) keep |= 1ull << l;
            }
            keep &= glhip::list_lanes(ng);
            int n = __builtin_popcountll(keep);
            if (n == 0) continue;
            unsigned long long todo = keep;
            int ring[4];
            for (int k = 0; k < 3; ++k) std::printf("A %d\n", ring[k] = glhip::list_pop(todo, g0, glast));
            for (int k = 0;; ++k) {
                std::printf("A %d\n", ring[(k + 3) & 3] = glhip::list_pop(todo, g0, glast));
                std::printf("C %d\n", ring[k & 3]);
                if (--n == 0) break;
            }
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("list_cursor")
    src = d / "list_cursor.cpp"
    src.write_text(PROGRAM)
    out = d / "list_cursor"
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", HEADER_DIR, str(src), "-o", str(out)]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True)
    if san.returncode != 0:      # a compiler without the sanitizer runtimes: the comparison is the same
        subprocess.run(base, check=True)
    return str(out)


def _play(exe, slots, ns, kept):
    text = f"{len(slots)} {ns} {len(kept)}\n" + " ".join(f"{a} {b}" for a, b in slots) + "\n" + " ".join(str(int(k)) for k in kept) + "\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    per_split, cur = {}, None
    for line in r.stdout.strip().split("\n"):
        tag, *v = line.split()
        if tag == "S":
            cur = per_split.setdefault(int(v[0]), {"B": [], "C": [], "A": []})
        elif tag == "B":
            cur["B"].append((int(v[0]), int(v[1])))
        else:
            cur[tag].append(int(v[0]))
    return per_split


def _check(exe, slots, ns, M, kept):
    nG = (M + 31) // 32
    got = _play(exe, slots, ns, kept)
    for split in range(ns):
        want, batches = [], []
        for a, b in slots[split::ns]:
            if b > a:
                groups = list(range(a // 32, (b + 31) // 32))
                want += [g for g in groups if kept[g]]
                batches += [(groups[k], min(64, len(groups) - k)) for k in range(0, len(groups), 64)]
        assert got[split]["C"] == want, (split, ns)
        assert got[split]["B"] == batches
        assert all(0 <= g < nG for g in got[split]["A"])


def _slots(rng, M, n_pieces, n_empty):
    """pieces of whole blocks of 256 columns (the last may end at M), ascending and disjoint, with empty slots mixed in"""
    nT = (M + 255) // 256
    cuts = np.sort(rng.choice(np.arange(1, nT), size=min(2 * n_pieces - 1, nT - 1), replace=False))
    edges = [0] + [int(c) for c in cuts] + [nT]
    pieces = [(256 * edges[k], min(M, 256 * edges[k + 1])) for k in range(0, len(edges) - 1, 2)]
    slots = pieces + [(0, 0)] * n_empty
    order = rng.permutation(len(slots))
    mixed = [slots[i] for i in order]
    return mixed + [(0, 0), (0, 0)]      # unused slots behind the last piece, zero-filled


@pytest.mark.parametrize("keep", ["random", "all", "none", "sparse"])
@pytest.mark.parametrize("ns", [1, 2, 3, 5])
def test_cursor_against_serial_walk(exe, ns, keep):
    rng = np.random.default_rng(100 * ns + len(keep))
    for M in (313000, 320037, 65536 + 8, 2048 * 5):
        nG = (M + 31) // 32
        kept = {"random": rng.random(nG) < 0.5, "all": np.ones(nG, bool), "none": np.zeros(nG, bool), "sparse": rng.random(nG) < 0.03}[keep]
        _check(exe, _slots(rng, M, 40, 7), ns, M, kept)


def test_piece_lengths_around_a_batch(exe):
    """pieces of 8, 64, 72, 128 and 136 groups (whole blocks), and a last piece that ends in a partial group"""
    M = 256 * 200 + 37
    rng = np.random.default_rng(5)
    kept = rng.random((M + 31) // 32) < 0.6
    slots = [(0, 256), (256 * 2, 256 * 10), (256 * 11, 256 * 20), (256 * 30, 256 * 46), (256 * 50, 256 * 67), (0, 0), (256 * 190, M)]
    for ns in (1, 2, 4):
        _check(exe, slots, ns, M, kept)
