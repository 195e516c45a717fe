"""Column-tile map of k_conv3x3_sp2p (alpha_zero_amd/csrc/az_conv_sp2p.h): the 2 x 80 positions of a PAIR of 9x9 boards (each without its
(8, 0) corner) in 10 column tiles x 16 lanes.  An entry is board * 81 + position.

Tiles 3, 5 and 6 are the edge tiles: row 0 / row 8 (columns 1-8) and column 0 (rows 0-7) of BOTH boards -- all 16 positions of such a tile
have 3 of the 9 taps off the board, and the kernel skips those MFMAs.  Tile 4 holds the same 8 positions of both boards; tiles 0-2 are
local to board A, tiles 7-9 (the same positions) to board B.

Bank rule of tools/gen_sp_map.py: lanes n in A = {0-3, 12-15} hit bank class cell(n) mod 16, lanes n in B = {4-11} class cell(n) + 8 mod 16,
and a tile is conflict-free iff the 16 classes are all different.  The second board's image lies a multiple of 256 B behind the first, so
a spanning tile with one board's 8 positions in the A lanes and the same 8 positions of the other board in the B lanes is conflict-free iff
the 8 cells differ mod 8.

Which of the remaining 56 positions (rows 1-7, columns 1-8) go where decides two things.
  Stores.  A lane pair stores the 16 bytes of one position and channel chunk; a chunk plane is 81 x 16 B, so a board row's columns 1-8 are 128
contiguous bytes, at every 16-byte alignment over the 16 chunks.  The L2 writes 64-byte granules (4 positions) back, 32-byte sectors
(2 positions) at the least: a granule whose positions sit in ONE tile is filled by one store instruction; one whose positions sit in several
tiles is filled piecemeal, units apart, and leaves the L2 once per piece if the line is evicted in between.  So the table keeps WHOLE ROWS
together: a row's 8 cells differ mod 8, hence a row is a valid spanning tile, and two rows form a conflict-free local tile iff their first
cells differ by an even number mod 16, that is iff the rows are an even number of rows apart (per class mod 8 the two cells are either equal
mod 16 -- one in the A lanes, one in the B lanes -- or a (c, c + 8) couple that shares a lane group, and the couples must split evenly).
  Fragment reads.  The B fragment of a local tile at tap row dy is the LDS data of the tile one board row lower at tap row dy - 1 -- if the
lower tile is the upper one shifted by a board row LANE FOR LANE.  Rows FOUR apart are the choice that lets the three local tiles be
row shifts of one another: tile 0 = rows (1, 5), tile 1 = tile 0 + 9 = rows (2, 6), tile 2 = tile 0 + 18 = rows (3, 7), and row 4 is the
spanning tile.  The kernel then reads one fragment per (row set, tap column, k-half) for all the tiles it feeds (the skewed k-step order).
A shift by a board row moves every cell by the pitch, hence every bank class by the same amount: the shifted tiles are conflict-free
because tile 0 is.

What stays free is the lane order of tile 0 -- which cell of an equal-class pair sits in the A lanes, which two of the four couples -- and which
board of the spanning tile has the A lanes: 192 tables that the rules above do not tell apart, one taken by the recorded seed.  Prints
the table as a C initializer with the number of sector-complete stores -- neighbouring positions (p, p + 1) of a board inside one tile: each
is one 32-byte sector stored whole in the chunks of one parity --; the header static_asserts the rules and the count again."""
import random

P, C0, S, CORNER = 11, 12, 9, 72
A = [0, 1, 2, 3, 12, 13, 14, 15]
B = [4, 5, 6, 7, 8, 9, 10, 11]
SEED = 66
BASE_ROWS, SPANNING_ROW = (1, 5), 4  # tile 0; tiles 1 and 2 are tile 0 one and two board rows lower


def cell(p):
    return C0 + P * (p // S) + p % S


TOP = [x for x in range(1, 9)]
BOTTOM = [8 * S + x for x in range(1, 9)]
LEFT = [y * S for y in range(8)]
ROWS = {y: [y * S + x for x in range(1, 9)] for y in range(1, 8)}


def base_tile(rng, ya, yb):
    """(A lanes' positions, B lanes' positions) of the tile made of rows ya and yb, the free choices drawn from rng"""
    a, b, couples = [], [], []
    for c in range(8):
        p, = [v for v in ROWS[ya] if cell(v) % 8 == c]
        q, = [v for v in ROWS[yb] if cell(v) % 8 == c]
        if cell(p) % 16 == cell(q) % 16:
            if rng.random() < 0.5:
                p, q = q, p
            a.append(p), b.append(q)
        else:
            couples.append((p, q))
    assert len(couples) % 2 == 0, "rows an even number of rows apart"
    in_a = set(rng.sample(range(len(couples)), len(couples) // 2))  # half of the couples in the A lanes, half in the B lanes
    for i, pq in enumerate(couples):
        (a if i in in_a else b).extend(pq)
    return sorted(a), sorted(b)


def lanes(a, b):
    row = [None] * 16
    for n, p in zip(A, a):
        row[n] = p
    for n, p in zip(B, b):
        row[n] = p
    return row


def spanning(pos8, flip=False):
    """board A's positions in the A lanes and board B's in the B lanes, or (flip) the other way round"""
    own, other = sorted(pos8), [81 + p for p in sorted(pos8)]
    return lanes(other, own) if flip else lanes(own, other)


def table(seed):
    for edge in (TOP, BOTTOM, LEFT):
        assert sorted(cell(p) % 8 for p in edge) == list(range(8)), edge
    assert all(sorted(cell(p) % 8 for p in r) == list(range(8)) for r in ROWS.values())
    rng = random.Random(seed)
    a, b = base_tile(rng, *BASE_ROWS)
    flip = rng.random() < 0.5
    local = [([p + S * j for p in a], [p + S * j for p in b]) for j in range(3)]
    rows = [lanes(a, b) for a, b in local]                                      # 0-2: board A
    rows += [spanning(TOP), spanning(ROWS[SPANNING_ROW], flip)]                 # 3, 4
    rows += [spanning(BOTTOM), spanning(LEFT)]                                  # 5, 6
    rows += [lanes([81 + p for p in a], [81 + p for p in b]) for a, b in local]   # 7-9: board B
    for row in rows:
        banks = sorted((cell(v % 81) + (8 if n in B else 0)) % 16 for n, v in enumerate(row))
        assert banks == list(range(16)), (row, banks)
    flat = sorted(v for row in rows for v in row)
    assert flat == sorted(b * 81 + p for b in range(2) for p in range(81) if p != CORNER)
    return rows


if __name__ == "__main__":
    rows = table(SEED)
    sector_complete = sum(1 for row in rows for v in row if v + 1 in row and v // 81 == (v + 1) // 81)
    print(f"    // generated by tools/gen_sp_map_pair.py (seed {SEED}; {sector_complete} sector-complete stores): board * 81 + position of (column tile, lane & 15)")
    for row in rows:
        print("    " + ", ".join(f"{v:3d}" for v in row) + ",")
