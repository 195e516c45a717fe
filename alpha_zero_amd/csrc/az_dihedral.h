// az_dihedral.h -- the eight board symmetries as index maps, shared by the flat transform kernels (azsp_impl.h: azsp_dihedral,
// azsp_replay_gather) and the engine's per-leaf symmetry (az_engine.h: write_features / expand_node).
//   D_op:  out[c][i][j] = in[c][az_dihedral_src(op, n, i, j)]     (utils/transformation.py:34-110)
// On a policy row D_op permutes the n * n board entries the same way and leaves the pass column alone.
#pragma once
#include "az_wave.h"

AZ_HD int az_dihedral_src(int op, int n, int i, int j) {
    int r, c;
    switch (op) {
        case 1: r = i; c = n - 1 - j; break;          // hflip: reverse the last dim (:46)
        case 2: r = n - 1 - i; c = j; break;          // vflip (:71)
        case 3: r = j; c = n - 1 - i; break;          // rot90 counter-clockwise (transformation_test.py:231-274)
        case 4: r = n - 1 - i; c = n - 1 - j; break;  // rot180
        case 5: r = n - 1 - j; c = i; break;          // rot270
        case 6: r = j; c = i; break;                  // transpose (extra)
        case 7: r = n - 1 - j; c = n - 1 - i; break;  // anti-transpose (extra)
        default: r = i; c = j; break;
    }
    return r * n + c;
}
// D_inv(op) undoes D_op: the two quarter turns swap, every other op is its own inverse.  As index maps src_inv(op) is the inverse
// permutation of src_op, so position p of the input of D_op lands at position az_dihedral_src(az_dihedral_inv(op), ...p) of its output.
AZ_HD int az_dihedral_inv(int op) { return op == 3 ? 5 : (op == 5 ? 3 : op); }
