"""The pair table of k_conv3x3_sp2p (alpha_zero_amd/csrc/az_conv_sp2p.h, tools/gen_sp_map_pair.py) without a GPU: the committed table is what
the generator prints for its recorded seed, it keeps the three hard rules the kernel is built on (re-implemented here, not imported), and
the number of 32-byte output sectors that one tile's store fills whole is the constant the header asserts."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "alpha_zero_amd", "csrc", "az_conv_sp2p.h")
S, P2, CORNER, PITCH, CELL0 = 9, 81, 72, 11, 12


def _header_table():
    hdr = open(HDR).read()
    body = hdr[hdr.index("constexpr Sp2pMap sp2p_map_table = {{"):]
    comment, rows = body[: body.index("}};")].split("\n", 2)[1:]
    tab = [int(v) for v in re.findall(r"\d+", rows)]
    assert len(tab) == 160
    return hdr, comment, [tab[16 * t:16 * t + 16] for t in range(10)]


def _tap_off(pos, tap):
    y, x = pos // S + tap // 3 - 1, pos % S + tap % 3 - 1
    return y < 0 or y >= S or x < 0 or x >= S


def test_committed_pair_table_is_the_generators_for_its_recorded_seed():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_sp_map_pair.py")], capture_output=True, text=True, check=True).stdout
    hdr, comment, tiles = _header_table()
    first, rest = out.split("\n", 1)
    assert first.strip() == comment.strip() and re.search(r"seed \d+", first)
    assert [int(v) for v in re.findall(r"\d+", rest)] == [v for t in tiles for v in t]


def test_pair_table_keeps_the_three_hard_rules():
    _, _, tiles = _header_table()
    # 1. every position of both boards but the two corners, once
    assert sorted(v for t in tiles for v in t) == [b * P2 + p for b in range(2) for p in range(P2) if p != CORNER]
    # 2. conflict-free lane groups: lanes 4-11 read 8 bank classes behind lanes 0-3 and 12-15; the 16 classes of a tile all differ
    for t in tiles:
        cls = sorted((CELL0 + PITCH * ((v % P2) // S) + (v % P2) % S + (8 if 4 <= n < 12 else 0)) % 16 for n, v in enumerate(t))
        assert cls == list(range(16)), t
    # 3. the three edge tiles and their 9 skipped (tile, tap) pairs, no other; the edge tiles are fixed sets
    skipped = {(j, tap) for j, t in enumerate(tiles) for tap in range(9) if all(_tap_off(v % P2, tap) for v in t)}
    assert skipped == {(3, 0), (3, 1), (3, 2), (5, 6), (5, 7), (5, 8), (6, 0), (6, 3), (6, 6)}
    both = lambda ps: sorted(ps + [P2 + p for p in ps])
    assert sorted(tiles[3]) == both(list(range(1, 9))) and sorted(tiles[5]) == both(list(range(73, 81))) and sorted(tiles[6]) == both([9 * y for y in range(8)])
    # the unit structure: tiles 0-2 board A only, 7-9 the same positions of board B, tile 4 the same 8 positions of both
    assert all(v < P2 for t in tiles[:3] for v in t) and [[v + P2 for v in t] for t in tiles[:3]] == tiles[7:]
    assert sorted(v + P2 for v in tiles[4] if v < P2) == sorted(v for v in tiles[4] if v >= P2) and len(set(tiles[4])) == 16


def test_sector_complete_count_is_the_headers_constant():
    """A 32-byte sector of the output holds two neighbouring positions of a board (which two depends on the chunk's parity: a chunk plane is
    81 x 16 B); a tile's store covers both parities, so every neighbouring pair (p, p + 1) inside one tile is one sector stored whole."""
    hdr, comment, tiles = _header_table()
    m = re.search(r"static_assert\(sp2p_sector_complete\(sp2p_map_table\) == (\d+)", hdr)
    if m is None:
        import pytest

        pytest.skip("the table was not regenerated for sector-complete stores")
    n = sum(1 for t in tiles for p in t if p + 1 in t and p // P2 == (p + 1) // P2)
    assert n == int(m.group(1)) and f"{n} sector-complete" in comment
