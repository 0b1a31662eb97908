// plan_source, box_nodes, ricker_weights: the host half of the source setters (source_tables.hpp).  Plain C++: no device,
// no HIP header.
#include "source_tables.hpp"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <unordered_map>

namespace sg {

SourcePlan plan_source(const SourceRequest& rq, int64_t nnz, const int64_t* nodes, int64_t nsteps, const double* values,
                       const double* weights) {
  SourcePlan pl;
  if (nnz < 0) throw std::invalid_argument("bad source request");
  if (nnz == 0 || nsteps == 0) return pl;
  if (!nodes || !values || nsteps < -1 || (weights && nsteps < 0)) throw std::invalid_argument("bad source request");
  const Layout& L = rq.L;
  const int d = rq.dim;
  const int64_t dd = (int64_t)d * d;
  pl.is_static = nsteps == -1;
  pl.nsteps = pl.is_static ? 1 : nsteps;
  const int64_t nslices = weights ? 1 : pl.nsteps;
  const int64_t nscalar = rq.ncells * L.nd;
  for (int64_t k = 0; k < nnz; ++k)
    if (nodes[k] < 0 || nodes[k] >= nscalar) throw std::invalid_argument("node index out of range");
  // A node listed more than once: its entries add up (in the order listed), merged here once so that every node is
  // written by one thread - the sum is then the same on every run and on every partition of the mesh (an atomic add
  // per entry gave the right sum in an arbitrary order, i.e. results that differed in the last bit from run to run).
  std::vector<int64_t> merged_nodes;
  std::vector<double> merged_values;
  {
    std::unordered_map<int64_t, int64_t> slot_of;
    slot_of.reserve((size_t)nnz * 2);
    std::vector<int64_t> to((size_t)nnz);
    for (int64_t k = 0; k < nnz; ++k) {
      auto it = slot_of.find(nodes[k]);
      if (it == slot_of.end()) {
        it = slot_of.emplace(nodes[k], (int64_t)merged_nodes.size()).first;
        merged_nodes.push_back(nodes[k]);
      }
      to[(size_t)k] = it->second;
    }
    if ((int64_t)merged_nodes.size() != nnz) {
      const int64_t nm = (int64_t)merged_nodes.size();
      merged_values.assign((size_t)(nslices * nm * dd), 0.0);
      for (int64_t s = 0; s < nslices; ++s)
        for (int64_t k = 0; k < nnz; ++k)
          for (int64_t c = 0; c < dd; ++c) merged_values[(size_t)((s * nm + to[(size_t)k]) * dd + c)] += values[(s * nnz + k) * dd + c];
      nodes = merged_nodes.data();
      values = merged_values.data();
      nnz = nm;
    }
  }
  pl.nnz = nnz;
  // Order the nodes so that those in cells of SG_REGION_FIRST come first: a split stage adds the
  // source to each part right after the launch that wrote it (the traces of FIRST are packed
  // before SECOND has run).  Then: device offset of component 0 of each node in the field layout.
  std::vector<int64_t> order((size_t)nnz);
  auto in_first = [&](int64_t node) {
    const int64_t cube = L.split(node).cube;
    const int64_t c[3] = {cube % rq.n[0], (cube / rq.n[0]) % rq.n[1], cube / ((int64_t)rq.n[0] * rq.n[1])};
    for (const Box& b : rq.first) {
      bool in = true;
      for (int k = 0; k < 3; ++k) in = in && c[k] >= b.o[k] && c[k] < b.o[k] + b.n[k];
      if (in) return true;
    }
    return false;
  };
  int64_t n1 = 0;
  for (int64_t i = 0; i < nnz; ++i)
    if (in_first(nodes[i])) order[(size_t)n1++] = i;
  pl.nfirst = n1;
  for (int64_t i = 0; i < nnz; ++i)
    if (!in_first(nodes[i])) order[(size_t)n1++] = i;
  pl.offs.resize((size_t)nnz);
  for (int64_t j = 0; j < nnz; ++j) {
    const Layout::Node at = L.split(nodes[order[(size_t)j]]);
    pl.offs[(size_t)j] = L.offset(at.cube, at.cls, at.b, dd, 0);
  }
  pl.vals.resize((size_t)(nslices * nnz * dd));
  for (int64_t k = 0; k < nslices; ++k)
    for (int64_t j = 0; j < nnz; ++j)
      std::copy_n(&values[(k * nnz + order[(size_t)j]) * dd], dd, &pl.vals[(size_t)((k * nnz + j) * dd)]);
  if (weights) pl.weights.assign(weights, weights + nsteps);
  if (rq.want_fused) {
    // tile kernels: item (gw = 16 squares of one class) -> slot, and per slot a dense (node, cell) -> value-row table, so
    // that the G stages add the source themselves (one launch less per G stage).  (Nodes are unique here: entries of a
    // node listed twice were merged above; one that were not would mean "not fused", not an error.)
    std::vector<int32_t> slot((size_t)L.item(rq.ncube_pad, 0), -1), idx;
    const size_t per_slot = (size_t)(L.nd * L.gw);
    bool dup = false;
    for (int64_t j = 0; j < nnz && !dup; ++j) {
      const Layout::Node at = L.split(nodes[order[(size_t)j]]);
      int32_t& s = slot[(size_t)L.item(at.cube, at.cls)];
      if (s < 0) {
        s = (int32_t)(idx.size() / per_slot);
        idx.resize(idx.size() + per_slot, -1);
      }
      int32_t& cell = idx[((size_t)s * L.nd + at.b) * L.gw + L.lane(at.cube)];
      dup = cell >= 0;
      cell = (int32_t)j;
    }
    if (!dup) {
      pl.slot.swap(slot);
      pl.idx.swap(idx);
    }
  }
  if (rq.sym)
    for (int64_t i = 0; i < nslices * nnz && pl.symmetric; ++i)
      for (int a = 0; a < d; ++a)
        for (int b = a + 1; b < d; ++b) pl.symmetric = pl.symmetric && pl.vals[i * dd + a * d + b] == pl.vals[i * dd + b * d + a];
  return pl;
}

std::vector<int64_t> box_nodes(const NodeGeom& G, const double* lo, const double* hi) {
  const sg_config& cfg = *G.cfg;
  const int d = G.d;
  // cubes that can hold a node of the box: those overlapping it (closed on both sides)
  int c0[3] = {0, 0, 0}, c1[3] = {0, 0, 0};
  for (int i = 0; i < d; ++i) {
    if (!(lo[i] <= hi[i])) throw std::invalid_argument("lo must not exceed hi");
    const double t0c = std::floor((lo[i] - cfg.origin[i]) / cfg.h[i]) - (double)cfg.cube0[i] - 1.0;
    const double t1c = std::floor((hi[i] - cfg.origin[i]) / cfg.h[i]) - (double)cfg.cube0[i] + 1.0;
    c0[i] = (int)std::max(0.0, std::min(t0c, (double)cfg.n[i]));
    c1[i] = (int)std::max(-1.0, std::min(t1c, (double)cfg.n[i] - 1.0));
  }
  std::vector<int64_t> nodes;
  for (int ck = c0[2]; ck <= c1[2]; ++ck)
    for (int cj = c0[1]; cj <= c1[1]; ++cj)
      for (int ci = c0[0]; ci <= c1[0]; ++ci) {
        const int c[3] = {ci, cj, ck};
        const int64_t cube = ci + (int64_t)cfg.n[0] * (cj + (int64_t)cfg.n[1] * ck);
        for (int k = 0; k < G.ncls; ++k)
          for (int b = 0; b < G.nq; ++b) {
            double x[3];
            G.node(c, k, b, x);
            bool in = true;
            for (int i = 0; i < d; ++i) in = in && x[i] >= lo[i] && x[i] <= hi[i];
            if (in) nodes.push_back((cube * G.ncls + k) * G.nq + b);
          }
      }
  return nodes;
}

std::vector<double> ricker_weights(double a, double t0, double t_first, double dt_step, int64_t nsteps) {
  std::vector<double> w((size_t)std::max<int64_t>(nsteps, 0));
  for (int64_t k = 0; k < nsteps; ++k) {
    const double t = t_first + (double)k * dt_step, q = (t - t0) * (t - t0);
    w[(size_t)k] = (-1.0 + 2.0 * a * q) * std::exp(-a * q);
  }
  return w;
}

}  // namespace sg
