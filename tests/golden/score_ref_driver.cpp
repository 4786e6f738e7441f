// TEST INFRASTRUCTURE ONLY -- drives the reference's UNMODIFIED lesson4 hector_mapping headers (compiled in place against
// oracle/shim/Eigen, never copied) for tests/golden/make_score_golden.py: a pyramid of GridMap levels built with the
// reference's own GridMap::updateByScan and DataContainer::setFrom, then OccGridMapUtil::getResidualForState,
// getLikelihoodForState, getCovarianceForPose and getCovMatrixWorldCoords on the recorder's (container, world pose, level)
// queries.  Everything numeric below is a call into the reference; this file only moves bytes.
//
//   score_ref_driver <in> <out> <reps>
// in : int32  n_levels, size_x, size_y, n_scans, n_queries
//      float  cell_length, offset_x, offset_y, occupied_factor
//      per scan:  int32 n; float pts[2n]; float pose_world[3]
//      per query: int32 kind (0 state, 1 covariance), level, n; float pts[2n] (level-0 cells); float pose_world[3]
// out: per level: float logodds[sy][sx]
//      per query: kind 0: float residual, likelihood
//                 kind 1: float likelihoods[7], cov_map[9], cov_world[9] (row-major)
//      double seconds per getLikelihoodForState call, best of <reps> passes over the kind-0 queries (0 when reps == 0)
#include <climits>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <vector>

#include <Eigen/Core>
#include <Eigen/Geometry>

#include "lesson4/hector_mapping/map/GridMap.h"
#include "lesson4/hector_mapping/map/OccGridMapUtilConfig.h"
#include "lesson4/hector_mapping/scan/DataPointContainer.h"

using hectorslam::DataContainer;
using hectorslam::GridMap;
typedef hectorslam::OccGridMapUtilConfig<GridMap> Util;

namespace {
struct Reader {
  std::vector<char> b;
  size_t at = 0;
  template <typename T>
  T get() {
    T v;
    std::memcpy(&v, b.data() + at, sizeof v);
    at += sizeof v;
    return v;
  }
};
struct Query {
  int kind, level;
  DataContainer dc;  // already scaled to the level by the reference's setFrom
  Eigen::Vector3f world;
};
void read_container(Reader& r, int n, DataContainer& dc) {
  dc.clear();
  dc.setOrigo(Eigen::Vector2f(0.f, 0.f));
  for (int i = 0; i < n; ++i) {
    const float x = r.get<float>(), y = r.get<float>();
    dc.add(Eigen::Vector2f(x, y));
  }
}
float level_factor(int level) { return static_cast<float>(1.0 / pow(2.0, static_cast<double>(level))); }  // MapRepMultiMap.h:161
}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  Reader r;
  {
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    fseek(f, 0, SEEK_END);
    r.b.resize((size_t)ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(r.b.data(), 1, r.b.size(), f) != r.b.size()) return 3;
    fclose(f);
  }
  const int reps = atoi(argv[3]);
  std::ostringstream sink;  // the reference prints from getCovarianceForPose
  std::streambuf* old = std::cout.rdbuf(sink.rdbuf());

  const int n_levels = r.get<int32_t>(), size_x = r.get<int32_t>(), size_y = r.get<int32_t>();
  const int n_scans = r.get<int32_t>(), n_queries = r.get<int32_t>();
  float cell = r.get<float>();
  const float off_x = r.get<float>(), off_y = r.get<float>(), occ = r.get<float>();
  std::vector<GridMap*> grids;
  std::vector<Util*> utils;
  {
    Eigen::Vector2i resolution(size_x, size_y);  // MapRepMultiMap.h:57-93
    for (int i = 0; i < n_levels; ++i) {
      grids.push_back(new GridMap(cell, resolution, Eigen::Vector2f(off_x, off_y)));
      grids.back()->setUpdateOccupiedFactor(occ);
      utils.push_back(new Util(grids.back()));
      resolution /= 2;
      cell *= 2.0f;
    }
  }
  DataContainer dc, scaled;
  for (int s = 0; s < n_scans; ++s) {
    const int n = r.get<int32_t>();
    read_container(r, n, dc);
    const float px = r.get<float>(), py = r.get<float>(), pt = r.get<float>();
    const Eigen::Vector3f pose(px, py, pt);
    for (int i = 0; i < n_levels; ++i) {  // MapRepMultiMap::updateByScan (:174-191) with matchData's containers (:161)
      if (i == 0) {
        grids[i]->updateByScan(dc, pose);
      } else {
        scaled.setFrom(dc, level_factor(i));
        grids[i]->updateByScan(scaled, pose);
      }
    }
  }
  for (int i = 0; i < n_levels; ++i) utils[i]->resetCachedData();  // the util caches cell probabilities (onMapUpdated, :127-135)

  std::vector<Query> qs((size_t)n_queries);
  for (int q = 0; q < n_queries; ++q) {
    qs[q].kind = r.get<int32_t>();
    qs[q].level = r.get<int32_t>();
    const int n = r.get<int32_t>();
    read_container(r, n, dc);
    if (qs[q].level == 0) qs[q].dc = dc;
    else qs[q].dc.setFrom(dc, level_factor(qs[q].level));
    const float px = r.get<float>(), py = r.get<float>(), pt = r.get<float>();
    qs[q].world = Eigen::Vector3f(px, py, pt);
  }

  FILE* out = fopen(argv[2], "wb");
  if (!out) return 4;
  for (int i = 0; i < n_levels; ++i) {
    const int n = grids[i]->getSizeX() * grids[i]->getSizeY();
    std::vector<float> lo((size_t)n);
    for (int c = 0; c < n; ++c) lo[c] = grids[i]->getCell(c).logOddsVal;
    fwrite(lo.data(), sizeof(float), lo.size(), out);
  }
  for (int q = 0; q < n_queries; ++q) {
    Query& Q = qs[q];
    Util& u = *utils[Q.level];
    const Eigen::Vector3f mp = u.getMapCoordsPose(Q.world);
    if (Q.kind == 0) {
      const float v[2] = {u.getResidualForState(mp, Q.dc), u.getLikelihoodForState(mp, Q.dc)};
      fwrite(v, sizeof(float), 2, out);
    } else {
      // the seven states, as getCovarianceForPose names them (OccGridMapUtil.h:252-278): it does not hand its likelihoods out
      const float dT = 1.5f, dA = 0.05f, x = mp[0], y = mp[1], a = mp[2];
      float v[25];
      v[0] = u.getLikelihoodForState(Eigen::Vector3f(x + dT, y, a), Q.dc);
      v[1] = u.getLikelihoodForState(Eigen::Vector3f(x - dT, y, a), Q.dc);
      v[2] = u.getLikelihoodForState(Eigen::Vector3f(x, y + dT, a), Q.dc);
      v[3] = u.getLikelihoodForState(Eigen::Vector3f(x, y - dT, a), Q.dc);
      v[4] = u.getLikelihoodForState(Eigen::Vector3f(x, y, a + dA), Q.dc);
      v[5] = u.getLikelihoodForState(Eigen::Vector3f(x, y, a - dA), Q.dc);
      v[6] = u.getLikelihoodForState(Eigen::Vector3f(x, y, a), Q.dc);
      const Eigen::Matrix3f cm = u.getCovarianceForPose(mp, Q.dc);
      const Eigen::Matrix3f cw = u.getCovMatrixWorldCoords(cm);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          v[7 + 3 * i + j] = cm(i, j);
          v[16 + 3 * i + j] = cw(i, j);
        }
      fwrite(v, sizeof(float), 25, out);
    }
  }
  double best = 0.0;
  if (reps > 0) {
    volatile float keep = 0.f;
    best = 1e30;
    for (int rep = 0; rep < reps; ++rep) {
      int calls = 0;
      const auto t0 = std::chrono::steady_clock::now();
      for (int q = 0; q < n_queries; ++q) {
        if (qs[q].kind != 0 || qs[q].dc.getSize() != 1081) continue;
        Util& u = *utils[qs[q].level];
        u.resetCachedData();  // a fresh map every call: what a caller scoring against a just-updated map pays
        keep = keep + u.getLikelihoodForState(u.getMapCoordsPose(qs[q].world), qs[q].dc);
        ++calls;
      }
      const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (calls > 0 && dt / calls < best) best = dt / calls;
    }
    if (best > 1e29) best = 0.0;
  }
  fwrite(&best, sizeof(double), 1, out);
  fclose(out);
  std::cout.rdbuf(old);
  return 0;
}
