// Is a node set of a lexicographic grid exactly a union of whole faces?  Plain host code without HIP types (compiles on its own).
#pragma once
#include <cstdint>

namespace poro {
// Grid of nn[0] x nn[1] x nn[2] nodes (nn[2] = 1 in 2D), node (i, j, k) at (k nn[1] + j) nn[0] + i; the set: the nodes whose mask byte has bit `bit`.
// fix[d][side] = 1 where every node of the face (direction d, side 0 = low / 1 = high) is in the set and allowed[d][side] is non-zero (0 rules a face out: not a
// physical boundary).  Returns whether the set equals the union of the flagged faces: every node is on a flagged face exactly when it is in the set.
inline bool whole_faces(const int64_t nn[3], int dim, const uint8_t *mask, int bit, const int allowed[3][2], int fix[3][2]) {
  auto in_set = [&](int64_t i, int64_t j, int64_t k) { return (mask[(k * nn[1] + j) * nn[0] + i] >> bit & 1) != 0; };
  for (int d = 0; d < 3; ++d) fix[d][0] = fix[d][1] = 0;
  for (int d = 0; d < dim; ++d) for (int side = 0; side < 2; ++side) {
    bool all = allowed[d][side] != 0;
    const int64_t fixed = side ? nn[d] - 1 : 0;
    const int d1 = (d + 1) % 3, d2 = (d + 2) % 3;
    for (int64_t a = 0; a < nn[d1] && all; ++a) for (int64_t b = 0; b < nn[d2]; ++b) {
      int64_t ix[3]; ix[d] = fixed; ix[d1] = a; ix[d2] = b;
      if (!in_set(ix[0], ix[1], ix[2])) { all = false; break; }
    }
    fix[d][side] = all ? 1 : 0;
  }
  for (int64_t k = 0; k < nn[2]; ++k) for (int64_t j = 0; j < nn[1]; ++j) for (int64_t i = 0; i < nn[0]; ++i) {
    const int64_t ix[3] = {i, j, k}; bool on = false;
    for (int d = 0; d < dim; ++d) on = on || (ix[d] == 0 && fix[d][0]) || (ix[d] == nn[d] - 1 && fix[d][1]);
    if (on != in_set(i, j, k)) return false;          // partial faces, interior nodes
  }
  return true;
}
}  // namespace poro
