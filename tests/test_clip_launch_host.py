"""gmr_amd/csrc/clip_launch.h without a GPU: a stand-alone C++ program (its own main, built with the host compiler under
AddressSanitizer and UBSan, never loaded into Python) reads one request per line -- a grid, an override with the variable it sets
first (setenv in the program), a body tree -- and prints what the header's functions give.  The tables are here, in Python:

- (a) every grid against the formulas of the commit before the header existed, written out again below (the `parent_*` functions);
- (b) the grids that can be worked out on paper, as literals;
- the overrides: which values are taken, which count as not set;
- the tree helpers on a chain, a star, two branches, 64 bodies and an order that is topological but not depth-first.

The limits that live in the kernel headers (kTrPairWaves, kTrMaxTile, kColPairsLdsMax, the targets) are read from those headers.
"""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gmr_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "clip_launch.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "slots") {  // target n_frames n_clips groups
      long long target, n_frames, n_clips; int groups;
      in >> target >> n_frames >> n_clips >> groups;
      printf("%u\n", gmr::clip_waves(target, n_clips, gmr::mean_clip_slots(n_frames, groups, n_clips)));
    } else if (op == "tiles") {  // target n_rows n_clips tile
      long long target, n_rows, n_clips; int tile;
      in >> target >> n_rows >> n_clips >> tile;
      printf("%u\n", gmr::clip_waves(target, n_clips, gmr::mean_clip_tiles(n_rows, n_clips, tile)));
    } else if (op == "footlock") {  // n_frames n_seq tile
      long long n_frames, n_seq; int tile;
      in >> n_frames >> n_seq >> tile;
      printf("%u\n", gmr::footlock_clip_waves(n_frames, n_seq, tile));
    } else if (op == "pair") {  // n_sources tile n_dst max_waves
      long long n_sources, n_dst, max_waves; int tile;
      in >> n_sources >> tile >> n_dst >> max_waves;
      printf("%u\n", gmr::transitions_pair_waves(n_sources, tile, n_dst, max_waves));
    } else if (op == "unsetenv") {  // name
      std::string name;
      in >> name;
      unsetenv(name.c_str());
      puts("ok");
    } else if (op == "setenv") {  // name, then the value: the rest of the line behind one blank (may be empty)
      std::string name, value;
      in >> name;
      std::getline(in, value);
      setenv(name.c_str(), value.empty() ? "" : value.c_str() + 1, 1);
      puts("ok");
    } else if (op == "int") {  // name lo hi unset
      std::string name; long lo, hi, unset;
      in >> name >> lo >> hi >> unset;
      printf("%ld\n", gmr::env_int(name.c_str(), lo, hi, unset));
    } else if (op == "lds") {  // name n_pairs lds_max
      std::string name; long long n_pairs, lds_max;
      in >> name >> n_pairs >> lds_max;
      printf("%d\n", gmr::collision_pairs_in_lds(name.c_str(), n_pairs, lds_max) ? 1 : 0);
    } else if (op == "tree") {  // the parents; arrays of exactly nbody entries, so that a write past them is caught
      std::vector<int32_t> parent;
      for (int p; in >> p;) parent.push_back(p);
      const int nb = (int)parent.size();
      std::vector<uint8_t> parent8(nb, 0x5a), depth8(nb, 0x5a);
      gmr::tree_parent_depth(parent.data(), nb, parent8.data(), depth8.data());
      printf("%d", gmr::tree_first_not_depth_first(parent.data(), nb));
      for (int b = 0; b < nb; ++b) printf(" %d:%d", (int)parent8[b], (int)depth8[b]);
      printf("\n");
    } else {
      fprintf(stderr, "unknown request: %s\n", line.c_str());
      return 2;
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(lines) -> the program's answers, one per request."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    d = tmp_path_factory.mktemp("clip_launch")
    src, exe = d / "clip_launch_test.cpp", d / "clip_launch_test"
    src.write_text(PROGRAM)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           f"-I{CSRC}", str(src), "-o", str(exe)])

    def run(lines):
        lines = list(lines)
        env = {k: v for k, v in os.environ.items() if not k.startswith("GMR_AMD_")}
        r = subprocess.run([str(exe)], input="".join(ln + "\n" for ln in lines), capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        answers = r.stdout.split("\n")[:-1]
        assert len(answers) == len(lines)
        return answers
    return run


def constant(header, name):
    text = open(os.path.join(CSRC, header)).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


K_FK_WAVE = constant("fk_kernel.hip.h", "kFkWave")
K_PAIR_WAVES = constant("transitions_kernel.hip.h", "kTrPairWaves")
K_MAX_TILE = constant("transitions_kernel.hip.h", "kTrMaxTile")
K_PAIRS_LDS_MAX = constant("self_collision_kernel.hip.h", "kColPairsLdsMax")


def test_the_kernel_headers_constants():
    """What the issue's literals and the rules below assume of them."""
    assert (K_FK_WAVE, K_PAIR_WAVES, K_MAX_TILE, K_PAIRS_LDS_MAX) == (64, 16384, 256, 4096)
    assert constant("dynamics_kernel.hip.h", "kDynTargetWaves") == constant("self_collision_kernel.hip.h", "kColTargetWaves") == 8192
    assert constant("transitions_kernel.hip.h", "kTrTargetWaves") == 8192
    assert constant("mirror_kernel.hip.h", "kMirrorTargetWaves") == constant("compose_kernel.hip.h", "kComposeTargetWaves") == 16384
    assert constant("mirror_kernel.hip.h", "kMirrorTile") == constant("compose_kernel.hip.h", "kComposeTile") == 64


# ---------------------------------------------------------------------------------------------------------------- (a) the restatement
# The launch arithmetic as api.hip spelled it before clip_launch.h, statement by statement (C++ integer division of non-negative
# numbers is Python's //).
def parent_slots(target, n_frames, n_seq, groups):   # dynamics_run, self_collision_run, transitions_run kernel a
    slots = (n_frames + groups - 1) // groups
    mean = (slots + n_seq - 1) // n_seq
    want = (target + n_seq - 1) // n_seq
    return max(1, min(min(want, mean), 65535))


def parent_tiles(target, n_rows, n_seq, tile):       # mirror_run, compose_run
    mean = (n_rows + n_seq - 1) // n_seq
    tiles = (mean + tile - 1) // tile
    want = (target + n_seq - 1) // n_seq
    return max(1, min(min(want, tiles), 65535))


def parent_window(target, n_frames, n_seq):          # transitions_run kernel b
    mean_b = ((n_frames + n_seq - 1) // n_seq + 64 - 1) // 64
    want = (target + n_seq - 1) // n_seq
    return max(1, min(min(want, mean_b), 65535))


def parent_footlock(n_frames, n_seq):                # footlock_run
    tiles = (n_frames + 64 - 1) // 64
    return min(min(tiles, 4 * ((tiles + n_seq - 1) // n_seq)), 65535)


def parent_pair(n_sources, tile, n_dst):             # transitions_run kernel c
    items = ((n_sources + tile - 1) // tile) * n_dst
    return max(1, min(items, 16384))


N_CLIPS = (1, 2, 3, 7, 2048, 8192, 20000, 100000)
MEAN_LENGTHS = (1, 5, 63, 64, 65, 300, 3000, 10 ** 6)
GROUPS = (1, 2, 4, 8)
TARGETS = (8192, 16384)


def test_grids_against_the_parents_formulas(ask):
    cases = []
    for n, mean, groups, target in itertools.product(N_CLIPS, MEAN_LENGTHS, GROUPS, TARGETS):
        for n_frames in {n * mean, max(1, n * mean - n // 2)}:   # every clip of the mean length, and a total that is no multiple
            tile = 32 * groups                                  # (kernel c's tile: 32 .. 256)
            cases += [(f"slots {target} {n_frames} {n} {groups}", parent_slots(target, n_frames, n, groups)),
                      (f"tiles {target} {n_frames} {n} 64", parent_tiles(target, n_frames, n, 64)),
                      (f"tiles {target} {n_frames} {n} {K_FK_WAVE}", parent_window(target, n_frames, n)),
                      (f"footlock {n_frames} {n} {K_FK_WAVE}", parent_footlock(n_frames, n)),
                      (f"pair {n_frames} {tile} {n} {K_PAIR_WAVES}", parent_pair(n_frames, tile, n))]
    assert len(cases) >= 5 * 8 * 8 * 4 * 2
    got = ask(c for c, _ in cases)
    wrong = [(c, int(g), want) for (c, want), g in zip(cases, got) if int(g) != want]
    assert not wrong, wrong[:10]
    assert all(1 <= int(g) <= 65535 for (c, _), g in zip(cases, got) if not c.startswith("pair"))


# ---------------------------------------------------------------------------------------------------------------- (b) the literals
LITERALS = [
    # wavefronts per clip, target 8192, frame slots: n_frames, n_seq, groups
    ("slots 8192 6144000 2048 2", 4),     # 2 048 clips x 3 000 frames: the case the header's comment promises
    ("slots 8192 100 1 2", 50),
    ("slots 8192 1000000 1 1", 8192),
    ("slots 8192 5 3 4", 1),
    # wavefronts per clip, target 16384, tiles of 64: n_frames, n_seq
    ("tiles 16384 1000 1 64", 16),
    (f"tiles 16384 {8192 * 300} 8192 64", 2),
    ("tiles 16384 10 3 64", 1),
    ("tiles 16384 20000 20000 64", 1),
    (f"tiles 16384 {20000 * 10 ** 6} 20000 64", 1),
    # foot locking: n_frames, n_seq
    ("footlock 4480000 1 64", 65535),
    ("footlock 6400 10 64", 40),
    ("footlock 64 5 64", 1),
    # kernel c: n_sources, tile, n_dst
    ("pair 1 64 1 16384", 1),
    ("pair 129 64 3 16384", 9),
    ("pair 1048577 64 1 16384", 16384),   # 16 385 items
    ("pair 6400 64 200 16384", 16384),    # 20 000 items
]


def test_grids_against_literals(ask):
    got = ask(c for c, _ in LITERALS)
    assert [int(g) for g in got] == [want for _, want in LITERALS]


# ---------------------------------------------------------------------------------------------------------------- the overrides
WAVE_VARIABLES = ("GMR_AMD_COLLISION_WAVES", "GMR_AMD_MIRROR_WAVES", "GMR_AMD_COMPOSE_WAVES", "GMR_AMD_TRANSITIONS_WAVES")


@pytest.mark.parametrize("name", WAVE_VARIABLES)
def test_wave_overrides(ask, name):
    ignored, taken = ["", "0", "-3", "65536", "abc"], [("1", 1), ("7", 7), ("65535", 65535), ("7x", 7)]
    lines = [f"unsetenv {name}", f"int {name} 1 65535 -1"]
    for v in ignored + [v for v, _ in taken]:
        lines += [f"setenv {name} {v}", f"int {name} 1 65535 -1"]
    lines += [f"unsetenv {name}", f"int {name} 1 65535 -1"]   # read on every call: unset again, ignored again
    got = [int(g) for g in ask(lines)[1::2]]
    assert got == [-1] + [-1] * len(ignored) + [want for _, want in taken] + [-1]


def test_overrides_of_other_ranges(ask):
    tile, taper = "GMR_AMD_TRANSITIONS_TILE", "GMR_AMD_BALANCE_TAPER"
    lines = [f"setenv {tile} 256", f"int {tile} 1 {K_MAX_TILE} 64", f"setenv {tile} 257", f"int {tile} 1 {K_MAX_TILE} 64",
             f"setenv {tile} 1", f"int {tile} 1 {K_MAX_TILE} 64", f"setenv {tile} 0", f"int {tile} 1 {K_MAX_TILE} 64",
             "int GMR_AMD_TRANSITIONS_WAVES 1 65535 0",                        # another variable: not set
             f"setenv {taper} 0", f"int {taper} 0 2147483647 16",                # a range that starts at 0 takes "0"
             f"setenv {taper} 2147483648", f"int {taper} 0 2147483647 16", f"setenv {taper} -1", f"int {taper} 0 2147483647 16"]
    got = ask(lines)
    assert [got[i] for i in (1, 3, 5, 7, 8, 10, 12, 14)] == ["256", "64", "1", "64", "0", "0", "16", "16"]


def test_collision_pairs_override(ask):
    name, small, big = "GMR_AMD_COLLISION_PAIRS", K_PAIRS_LDS_MAX, K_PAIRS_LDS_MAX + 1
    q = [f"lds {name} 1 {K_PAIRS_LDS_MAX}", f"lds {name} {small} {K_PAIRS_LDS_MAX}", f"lds {name} {big} {K_PAIRS_LDS_MAX}"]
    lines = [f"unsetenv {name}"] + q
    for v in ("global", "g", "lds", "", "Global"):
        lines += [f"setenv {name} {v}"] + q
    got = ask(lines)
    rows = [[int(g) for g in got[i + 1:i + 4]] for i in range(0, len(got), 4)]
    assert rows == [[1, 1, 0],    # not set: LDS where the table fits
                    [0, 0, 0],    # global forces global
                    [0, 0, 0],    # (its first letter decides)
                    [1, 1, 0],    # lds: only where it fits -- a table larger than kColPairsLdsMax stays global
                    [1, 1, 0],
                    [1, 1, 0]]    # (a capital G is not 'g', as before)


# ---------------------------------------------------------------------------------------------------------------- the tree helpers
def tree(ask, parents):
    first, *cells = ask(["tree " + " ".join(str(p) for p in parents)])[0].split()
    return int(first), [tuple(int(x) for x in c.split(":")) for c in cells]


def depths(parents):
    d = []
    for p in parents:
        d.append(0 if p < 0 else d[p] + 1)
    return d


@pytest.mark.parametrize("parents", [
    [-1],
    [-1, 0, 1, 2, 3, 4],                              # a chain
    [-1, 0, 0, 0, 0, 0],                              # a star
    [-1, 0, 1, 2, 0, 4, 5, 5],                        # two branches, the second forks again
    [-1] + list(range(63)),                           # 64 bodies in a chain: depth 63
    [-1] + [0] * 63,                                  # 64 bodies in a star
], ids=["root", "chain", "star", "branches", "chain64", "star64"])
def test_tree_parent_depth(ask, parents):
    first, cells = tree(ask, parents)
    assert first == 0                                 # depth-first: nothing to refuse
    assert cells[0] == (0xff, 0)
    assert cells == [(0xff if p < 0 else p, d) for p, d in zip(parents, depths(parents))]


def test_two_branches_literally(ask):
    first, cells = tree(ask, [-1, 0, 1, 0, 3, 3])
    assert first == 0
    assert cells == [(255, 0), (0, 1), (1, 2), (0, 1), (3, 2), (3, 2)]


@pytest.mark.parametrize("parents, body", [
    ([-1, 0, 0, 1], 3),                               # body 3 hangs on body 1 after body 2 was opened
    ([-1, 0, 1, 0, 2], 4),                            # back into a closed subtree
    ([-1, 0, 1, 2, 1, 2], 5),
])
def test_topological_but_not_depth_first(ask, parents, body):
    """Every parent precedes its child -- what model creation checks -- so parents and depths are right, and the depth-first test names
    the first body that does not follow its parent's subtree, as gmr_motion_dynamics reports it."""
    assert all(0 <= p < b for b, p in enumerate(parents) if b)
    first, cells = tree(ask, parents)
    assert first == body
    assert cells == [(0xff if p < 0 else p, d) for p, d in zip(parents, depths(parents))]


def test_header_is_host_only():
    """Plain C++ with no HIP include, as the stand-alone build above needs."""
    text = open(os.path.join(CSRC, "clip_launch.h")).read()
    assert "hip" not in "\n".join(ln for ln in text.split("\n") if ln.lstrip().startswith("#include"))


def test_api_uses_the_header():
    """The launch arithmetic is written once: api.hip parses no number from the environment itself."""
    text = open(os.path.join(CSRC, "api.hip")).read()
    assert '#include "clip_launch.h"' in text and "strtol" not in text
    for name in WAVE_VARIABLES + ("GMR_AMD_TRANSITIONS_TILE", "GMR_AMD_COLLISION_PAIRS"):
        assert text.count(f'"{name}"') == 1, name
