"""The skewed k-step order of k_conv3x3_sp2p (alpha_zero_amd/csrc/az_conv_sp2p.h) without a GPU: an independent restatement, from the table
in the header, of which (tile, tap, k-half) a unit multiplies in which step and which B fragments it requests.

U0 (tiles 0-2) and U3 (tiles 8, 9) hold tiles that are row shifts of one another: the fragment of tile j at tap row dy is the LDS data of the
unit's first tile at tap row j + dy, so a step (row set s, tap column dx, k-half) reads ONE fragment pair for every tile j with s - j in -1..1.
U1 (tiles 3, 4) and U2 (tiles 5-7) read a fragment per live tile in the plain order (tap, k-half).  Checked: the table's shifts; per unit the
steps, each live (tile, tap, k-half) exactly once and per tile in ascending weight k-step (the accumulation chain of the plain order, hence the
same words); 972 MFMAs and 252 fragment requests per wave and pair, the numbers the header asserts; a request per MFMA gap."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "alpha_zero_amd", "csrc", "az_conv_sp2p.h")
S, P2 = 9, 81
UNITS = ((0, 1, 2), (3, 4), (5, 6, 7), (8, 9))


def _header():
    hdr = open(HDR).read()
    body = hdr[hdr.index("constexpr Sp2pMap sp2p_map_table = {{"):]
    tab = [int(v) for v in re.findall(r"\d+", body[: body.index("}};")].split("\n", 2)[2])]
    assert len(tab) == 160
    return hdr, [tab[16 * t:16 * t + 16] for t in range(10)]


def _skipped(tile, tap):
    """the tap is off the board for all 16 positions of the tile"""
    def off(pos):
        y, x = pos // S + tap // 3 - 1, pos % S + tap % 3 - 1
        return y < 0 or y >= S or x < 0 or x >= S
    return all(off(v % P2) for v in tile)


def _row_shifts(tiles, unit):
    base = tiles[unit[0]]
    return all(tiles[j] == [v + S * k for v in base] for k, j in enumerate(unit)) and not any(_skipped(tiles[j], tap) for j in unit for tap in range(9))


def _steps(tiles, unit):
    """[(fragments requested for the step, [(tile, tap, k-half), ...])] in the order the unit runs them"""
    steps = []
    if _row_shifts(tiles, unit):
        for s in range(-1, len(unit) + 1):  # the row set: the rows of the unit's first tile, s board rows lower
            for dx in (-1, 0, 1):
                for kh in (0, 1):
                    live = [(j, (s - k + 1) * 3 + dx + 1, kh) for k, j in enumerate(unit) if -1 <= s - k <= 1]
                    steps.append((1, live))
    else:
        for tap in range(9):
            for kh in (0, 1):
                live = [(j, tap, kh) for j in unit if not _skipped(tiles[j], tap)]
                steps.append((len(live), live))
    return steps


def test_local_tiles_are_row_shifts_and_the_spanning_tile_is_one_row_of_both_boards():
    _, tiles = _header()
    assert tiles[1] == [v + 9 for v in tiles[0]] and tiles[2] == [v + 18 for v in tiles[0]]
    assert tiles[7:] == [[v + P2 for v in t] for t in tiles[:3]]
    a, b = sorted(v for v in tiles[4] if v < P2), sorted(v - P2 for v in tiles[4] if v >= P2)
    assert a == b and len(a) == 8 and len({p // S for p in a}) == 1 and sorted(p % S for p in a) == list(range(1, 9))
    assert [_row_shifts(tiles, u) for u in UNITS] == [True, False, False, True]
    # the rows of a local tile are four apart: the only spacing at which three tiles are shifts of one and row 4 is left for the spanning tile
    assert sorted({v // S for v in tiles[0]}) == [1, 5] and a[0] // S == 4


def test_skewed_steps_multiply_every_live_tap_once_in_ascending_weight_order():
    _, tiles = _header()
    live_tiles_per_row_set = []
    for unit in UNITS:
        steps = _steps(tiles, unit)
        seen = [m for _, live in steps for m in live]
        want = [(j, tap, kh) for j in unit for tap in range(9) for kh in (0, 1) if not _skipped(tiles[j], tap)]
        assert sorted(seen) == sorted(want) and len(set(seen)) == len(seen), unit  # each live (tile, tap, k-half) exactly once
        for j in unit:  # a tile's accumulators meet its weight k-steps (tap * 2 + k-half) in ascending order
            ks = [tap * 2 + kh for jj, tap, kh in seen if jj == j]
            assert ks == sorted(ks), (unit, j, ks)
        assert all(live for _, live in steps), unit  # no empty step
        live_tiles_per_row_set.append([len(live) for _, live in steps][::6] if _row_shifts(tiles, unit) else None)
    assert live_tiles_per_row_set == [[1, 2, 3, 2, 1], None, None, [1, 2, 2, 1]]
    assert [len(_steps(tiles, u)) for u in UNITS] == [30, 18, 18, 24]


def test_mfma_and_fragment_counts_are_the_headers():
    hdr, tiles = _header()
    mfmas = [6 * sum(len(live) for _, live in _steps(tiles, u)) for u in UNITS]  # 2 cout tiles x 3 products per (tile, tap, k-half)
    reads = [2 * sum(n for n, _ in _steps(tiles, u)) for u in UNITS]            # a fragment is a hi and a lo plane
    assert sum(mfmas) == 972 and mfmas == [324, 180, 252, 216]
    assert sum(reads) == 252 and reads == [60, 60, 84, 48]
    assert "Sp2pU<0>::S.n + Sp2pU<1>::S.n + Sp2pU<2>::S.n + Sp2pU<3>::S.n == 972" in hdr
    m = re.search(r"static_assert\(Sp2pU<0>::S\.reads\(\) == (\d+) && Sp2pU<1>::S\.reads\(\) == (\d+) && Sp2pU<2>::S\.reads\(\) == (\d+) && Sp2pU<3>::S\.reads\(\) == (\d+),", hdr)
    assert m and [int(v) for v in m.groups()] == reads


def test_a_steps_fragments_fit_the_mfma_gaps_of_its_predecessor():
    """The fragments of a step are requested in the gaps behind the MFMAs of the step before it (the last step of a unit requests the first
    step of the next unit, U3's last step U0's first), one ds_read_b128 per gap: 2 reads per fragment against 6 MFMAs per live tile."""
    _, tiles = _header()
    seq = [st for u in UNITS for st in _steps(tiles, u)]
    for prev, (nfrag, _) in zip(seq, seq[1:] + seq[:1]):
        assert 2 * nfrag <= 6 * len(prev[1]), (prev, nfrag)
