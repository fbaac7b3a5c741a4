// Face tables of the Kelly error indicator (poro_pres_estimate_error), host side and free of HIP: shared by the device library (ctx_adapt.hip uploads them) and by the
// host layer, whose CPU test checks them against a model without a GPU.
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace poro {

// faces sorted by their first cell: cell_a / cell_b / code per face (code: kernels_kelly.hip), and per cell the entries ent_ptr[c] .. ent_ptr[c + 1] = (face, cell whose
// diameter scales it) in the order of the cell's local faces
struct KellyTables { std::vector<int32_t> cell_a, cell_b, code, ent_face, ent_hcell; std::vector<int64_t> ent_ptr; };

// Interior faces of the mesh from the cells' pressure dofs (one per vertex), the boundary-face list and the hanging-node constraints of the pressure space:
//   - a face two cells share (same sorted vertex tuple) is a regular face;
//   - a face of one cell only that is in the boundary-face list is a boundary face (no contribution);
//   - every other face of one cell only belongs to a hanging face: a FINE face has hanging vertices, and the masters of those together with its one
//     unconstrained vertex (the corner it shares) are the corners of the COARSE face it lies in; a coarse face has 2^(dim-1) such subfaces.
// Anything else is refused.
inline KellyTables build_kelly_tables_host(int dim, int64_t nc, int64_t n_p, const std::vector<int32_t> &cv /* [nc][2^dim] pressure dofs */, int64_t n_bfaces, const std::vector<int32_t> &bfc,
                                           const std::vector<int32_t> &bfl, int64_t n_cons, const std::vector<int32_t> &hdof, const std::vector<int64_t> &hptr, const std::vector<int32_t> &hmaster,
                                           const std::vector<double> &hw) {
  const int nv = 1 << dim, nfv = nv / 2, nf = 2 * dim;
  std::vector<int64_t> cons_of((size_t)n_p, -1);
  for (int64_t i = 0; i < n_cons; ++i) cons_of[hdof[i]] = i;
  auto face_vertex = [&](int f, int j) { const int d = f >> 1, side = f & 1; return (j & ((1 << d) - 1)) | (side << d) | ((j >> d) << (d + 1)); };   // local vertex j of local face f
  typedef std::array<int32_t, 4> Key;
  auto sorted_key = [&](const int32_t *v) { Key k{INT_MAX, INT_MAX, INT_MAX, INT_MAX}; for (int j = 0; j < nfv; ++j) k[j] = v[j]; std::sort(k.begin(), k.begin() + nfv); return k; };
  struct Rec { Key key; int32_t cell, f; };
  std::vector<Rec> all((size_t)nc * nf);
  for (int64_t e = 0; e < nc; ++e) for (int f = 0; f < nf; ++f) {
    int32_t v[4] = {0, 0, 0, 0}; for (int j = 0; j < nfv; ++j) v[j] = cv[e * nv + face_vertex(f, j)];
    all[(size_t)e * nf + f] = Rec{sorted_key(v), (int32_t)e, f};
  }
  std::sort(all.begin(), all.end(), [](const Rec &a, const Rec &b) { return a.key != b.key ? a.key < b.key : a.cell != b.cell ? a.cell < b.cell : a.f < b.f; });
  std::vector<uint8_t> is_bface((size_t)nc * nf, 0);
  for (int64_t i = 0; i < n_bfaces; ++i) { if (bfc[i] < 0 || bfc[i] >= nc || bfl[i] < 0 || bfl[i] >= nf) throw std::runtime_error("kelly: boundary face out of range"); is_bface[(size_t)bfc[i] * nf + bfl[i]] = 1; }

  struct Face { int32_t a, b, fa, fb, hcell_a, hcell_b; int ref_b[4][3]; };
  std::vector<Face> faces;
  // twice the reference coordinates in cell b of the dof `id` when it is one of b's vertices
  auto vertex_ref = [&](int32_t b, int32_t id, int out[3]) { for (int lv = 0; lv < nv; ++lv) if (cv[(int64_t)b * nv + lv] == id) { for (int k = 0; k < 3; ++k) out[k] = k < dim ? 2 * ((lv >> k) & 1) : 0; return true; } return false; };
  std::map<Key, std::pair<int32_t, int32_t>> coarse;      // faces of one cell without hanging vertices, not on the boundary: candidates for the coarse side
  std::map<Key, int> coarse_count;
  std::vector<std::pair<int32_t, int32_t>> fine;
  for (size_t i = 0; i < all.size();) {
    size_t j = i + 1; while (j < all.size() && all[j].key == all[i].key) ++j;
    if (j - i > 2) throw std::runtime_error("kelly: more than two cells share a face");
    if (j - i == 2) {
      if (all[i].cell == all[i + 1].cell) throw std::runtime_error("kelly: a cell has the same face twice");
      Face F{}; F.a = all[i].cell; F.fa = all[i].f; F.b = all[i + 1].cell; F.fb = all[i + 1].f; F.hcell_a = F.a; F.hcell_b = F.b;
      for (int q = 0; q < nfv; ++q) if (!vertex_ref(F.b, cv[(int64_t)F.a * nv + face_vertex(F.fa, q)], F.ref_b[q])) throw std::runtime_error("kelly: face vertices do not match");
      faces.push_back(F);
    } else if (!is_bface[(size_t)all[i].cell * nf + all[i].f]) {
      bool hanging = false; for (int q = 0; q < nfv; ++q) hanging = hanging || cons_of[all[i].key[q]] >= 0;
      if (hanging) fine.emplace_back(all[i].cell, all[i].f);
      else { coarse[all[i].key] = {all[i].cell, all[i].f}; coarse_count[all[i].key] = 0; }
    }
    i = j;
  }
  for (auto &ff : fine) {
    const int32_t a = ff.first; const int fa = ff.second;
    int32_t corners[16]; int n_corners = 0, n_free = 0;
    auto add = [&](int32_t id) { for (int q = 0; q < n_corners; ++q) if (corners[q] == id) return; if (n_corners < 16) corners[n_corners++] = id; };
    for (int q = 0; q < nfv; ++q) {
      const int32_t id = cv[(int64_t)a * nv + face_vertex(fa, q)]; const int64_t ci = cons_of[id];
      if (ci < 0) { add(id); ++n_free; } else for (int64_t k = hptr[ci]; k < hptr[ci + 1]; ++k) add(hmaster[k]);
    }
    const std::string where = " (cell " + std::to_string(a) + ", face " + std::to_string(fa) + ")";
    if (n_free != 1 || n_corners != nfv) throw std::runtime_error("kelly: a face with hanging vertices is not a subface of one coarse face" + where + ": meshes with one level of hanging nodes only");
    auto it = coarse.find(sorted_key(corners));
    if (it == coarse.end()) throw std::runtime_error("kelly: no coarse face matches the masters of a hanging face" + where);
    Face F{}; F.a = a; F.fa = fa; F.b = it->second.first; F.fb = it->second.second; F.hcell_a = F.b; F.hcell_b = F.b;   // deal.II takes the factor of both sides from the coarse cell
    for (int q = 0; q < nfv; ++q) {
      const int32_t id = cv[(int64_t)a * nv + face_vertex(fa, q)]; const int64_t ci = cons_of[id];
      if (ci < 0) { if (!vertex_ref(F.b, id, F.ref_b[q])) throw std::runtime_error("kelly: hanging face does not touch its coarse face" + where); continue; }
      double r[3] = {0, 0, 0}, wsum = 0;
      for (int64_t k = hptr[ci]; k < hptr[ci + 1]; ++k) { int m[3]; if (!vertex_ref(F.b, hmaster[k], m)) throw std::runtime_error("kelly: a master is not a vertex of the coarse cell" + where); for (int d = 0; d < 3; ++d) r[d] += hw[k] * m[d]; wsum += hw[k]; }
      if (std::fabs(wsum - 1.0) > 1e-9) throw std::runtime_error("kelly: hanging-node weights do not sum to 1" + where);
      for (int d = 0; d < 3; ++d) { const double t = std::round(r[d]); if (std::fabs(r[d] - t) > 1e-9 || t < 0 || t > 2) throw std::runtime_error("kelly: hanging node is not a midpoint of its coarse face" + where); F.ref_b[q][d] = (int)t; }
    }
    for (int q = 0; q < nfv; ++q) if (F.ref_b[q][F.fb >> 1] != 2 * (F.fb & 1)) throw std::runtime_error("kelly: hanging face does not lie in its coarse face" + where);
    coarse_count[it->first]++;
    faces.push_back(F);
  }
  for (auto &kv : coarse_count) if (kv.second != nfv) {
    const auto &cf = coarse.at(kv.first);
    throw std::runtime_error("kelly: face " + std::to_string(cf.second) + " of cell " + std::to_string(cf.first) + " has no neighbour, is not a boundary face and is not covered by " + std::to_string(nfv) + " hanging subfaces");
  }
  // face order: by first cell (neighbouring lanes gather neighbouring cells), then its local face, then the second cell
  std::sort(faces.begin(), faces.end(), [](const Face &x, const Face &y) { return x.a != y.a ? x.a < y.a : x.fa != y.fa ? x.fa < y.fa : x.b < y.b; });
  const int64_t n_faces = (int64_t)faces.size();
  std::vector<int32_t> ha(n_faces), hb(n_faces), hcode(n_faces);
  struct Ent { int32_t cell, f, face, hcell; };
  std::vector<Ent> ents; ents.reserve((size_t)2 * n_faces);
  for (int64_t i = 0; i < n_faces; ++i) {
    const Face &F = faces[i]; int32_t code = F.fa | (F.fb << 27);
    for (int q = 0; q < nfv; ++q) for (int k = 0; k < dim; ++k) code |= F.ref_b[q][k] << (3 + 2 * (3 * q + k));
    ha[i] = F.a; hb[i] = F.b; hcode[i] = code;
    ents.push_back(Ent{F.a, F.fa, (int32_t)i, F.hcell_a}); ents.push_back(Ent{F.b, F.fb, (int32_t)i, F.hcell_b});
  }
  std::sort(ents.begin(), ents.end(), [](const Ent &x, const Ent &y) { return x.cell != y.cell ? x.cell < y.cell : x.f != y.f ? x.f < y.f : x.face < y.face; });
  std::vector<int64_t> eptr((size_t)nc + 1, 0); std::vector<int32_t> eface(ents.size()), ehcell(ents.size());
  for (size_t e = 0; e < ents.size(); ++e) { eptr[ents[e].cell + 1]++; eface[e] = ents[e].face; ehcell[e] = ents[e].hcell; }
  for (int64_t e = 0; e < nc; ++e) eptr[e + 1] += eptr[e];
  KellyTables T;
  T.cell_a = std::move(ha); T.cell_b = std::move(hb); T.code = std::move(hcode); T.ent_ptr = std::move(eptr); T.ent_face = std::move(eface); T.ent_hcell = std::move(ehcell);
  return T;
}

}  // namespace poro
