// 1DSfM keypoints/tracks ingestion and the CalcCovariance driver: the caller of the batched per-edge covariance kernel
// (SURVEY 8f rows 2 and 4).  Follows thirdparty/TheiaSfM/src/theia/io/read_1dsfm.cc:93-292 for the file formats and
// src/uncertainty.cpp:3-33,82-198 + bind_src/GlobalSfMpy.cpp:623-628 for what is estimated and written.
#include <glob.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>

#include "../../include/gsfm/view_graph.hpp"
#include "../../include/gsfm_rot.h"
#include "../../include/gsfm_tracks.h"
#include "../../include/gsfm_ba.h"
#include "../../include/gsfm_ba6.h"
#include "../../include/gsfm_ba7.h"

namespace gsfm {

namespace {
void AngleAxisToRowMajorMatrix(const double* a, double* R) {  // ceres::AngleAxisToRotationMatrix semantics
  const double t2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
  if (t2 > 2.220446049250313e-16) {
    const double t = std::sqrt(t2), wx = a[0] / t, wy = a[1] / t, wz = a[2] / t, c = std::cos(t), s = std::sin(t), k = 1.0 - c;
    R[0] = c + wx * wx * k; R[1] = wx * wy * k - wz * s; R[2] = wy * s + wx * wz * k;
    R[3] = wz * s + wx * wy * k; R[4] = c + wy * wy * k; R[5] = -wx * s + wy * wz * k;
    R[6] = -wy * s + wx * wz * k; R[7] = wx * s + wy * wz * k; R[8] = c + wz * wz * k;
  } else {
    R[0] = 1; R[1] = -a[2]; R[2] = a[1]; R[3] = a[2]; R[4] = 1; R[5] = -a[0]; R[6] = -a[1]; R[7] = a[0]; R[8] = 1;
  }
}
}  // namespace

bool Read1DSFMTracks(const std::string& dir, Tracks1DSfM* out, std::string* error) {
  *out = Tracks1DSfM();
  std::unordered_set<theia::ViewId> cc;
  {
    std::ifstream f(dir + "/cc.txt");
    theia::ViewId v;
    while (f >> v) cc.insert(v);
  }
  {
    // list.txt: "<image path>[ 0 <focal>]" per line; the view id is the line index (read_1dsfm.cc:114-163).
    std::ifstream f(dir + "/list.txt");
    if (!f.is_open()) { if (error) *error = "cannot read " + dir + "/list.txt"; return false; }
    std::string line;
    theia::ViewId id = 0;
    while (std::getline(f, line)) {
      std::istringstream ss(line);
      std::string name;
      if (!(ss >> name)) continue;
      int flag = 0;
      double focal = 0.0;
      if (!(ss >> flag >> focal)) focal = 0.0;
      if (cc.empty() || cc.count(id)) {
        out->focal[id] = focal;
        const size_t slash = name.find_last_of('/');
        out->names[id] = slash == std::string::npos ? name : name.substr(slash + 1);
      }
      ++id;
    }
  }
  {
    // coords.txt: "#index = I, name = N, keys = K, px = X, py = Y, focal = F" then K lines "k x y 0 0 r g b" (:165-230).
    std::ifstream f(dir + "/coords.txt");
    if (!f.is_open()) { if (error) *error = "cannot read " + dir + "/coords.txt"; return false; }
    std::string line;
    while (std::getline(f, line)) {
      if (line.empty()) continue;
      unsigned id = 0;
      int keys = 0;
      float px = 0, py = 0, fl = 0;
      char name[1024];
      if (std::sscanf(line.c_str(), "#index = %u, name = %1023s keys = %d, px = %f, py = %f, focal = %f", &id, name, &keys, &px, &py, &fl) < 3) {
        if (error) *error = "malformed coords.txt header: " + line;
        return false;
      }
      const bool keep = out->focal.count(id) != 0;
      std::vector<Eigen::Vector2d>* kp = nullptr;
      if (keep) {
        out->principal_point[id] = Eigen::Vector2d(px, py);
        kp = &out->keypoints[id];
        kp->reserve(keys);
      }
      for (int k = 0; k < keys; ++k) {
        if (!std::getline(f, line)) { if (error) *error = "coords.txt ends inside a key list"; return false; }
        if (!keep) continue;
        double x = 0, y = 0;
        if (std::sscanf(line.c_str(), "%*d %lf %lf", &x, &y) != 2) { if (error) *error = "malformed coords.txt key: " + line; return false; }
        kp->emplace_back(x, y);
      }
    }
  }
  {
    // tracks.txt: "<num tracks>" then per track "<len> (<view> <key>)*len" (:232-292).
    std::ifstream f(dir + "/tracks.txt");
    if (!f.is_open()) { if (error) *error = "cannot read " + dir + "/tracks.txt"; return false; }
    size_t n = 0;
    f >> n;
    out->tracks.reserve(n);
    for (size_t t = 0; t < n; ++t) {
      int len = 0;
      if (!(f >> len)) { if (error) *error = "tracks.txt is shorter than its header says"; return false; }
      std::vector<std::pair<theia::ViewId, int>> tr;
      tr.reserve(len);
      for (int k = 0; k < len; ++k) {
        theia::ViewId v;
        int key;
        if (!(f >> v >> key)) { if (error) *error = "tracks.txt ends inside a track"; return false; }
        const auto it = out->keypoints.find(v);
        if (it == out->keypoints.end()) continue;  // view outside the component
        if (key < 0 || (size_t)key >= it->second.size()) { if (error) *error = "tracks.txt references a missing keypoint"; return false; }
        tr.emplace_back(v, key);
      }
      out->tracks.push_back(std::move(tr));
    }
  }
  return true;
}

void CollectEdgeMatches(const Tracks1DSfM& tr, const theia::ViewGraph& vg, EdgeMatches* out) {
  *out = EdgeMatches();
  for (const auto& e : vg.GetAllEdges()) out->edges.push_back(e.first);
  std::sort(out->edges.begin(), out->edges.end());
  const size_t E = out->edges.size();
  std::unordered_map<theia::ViewIdPair, size_t> slot;
  slot.reserve(E * 2);
  for (size_t e = 0; e < E; ++e) slot[out->edges[e]] = e;

  // two passes over the tracks (count, fill): every pair of observations of one track whose views share an edge is a match
  std::vector<uint64_t> count(E + 1, 0);
  auto for_each_match = [&](auto&& fn) {
    for (const auto& t : tr.tracks)
      for (size_t a = 0; a < t.size(); ++a)
        for (size_t b = a + 1; b < t.size(); ++b) {
          if (t[a].first == t[b].first) continue;
          const bool swap = t[a].first > t[b].first;
          const auto& lo = swap ? t[b] : t[a];
          const auto& hi = swap ? t[a] : t[b];
          const auto it = slot.find(theia::ViewIdPair(lo.first, hi.first));
          if (it != slot.end()) fn(it->second, lo, hi);
        }
  };
  for_each_match([&](size_t e, const std::pair<theia::ViewId, int>&, const std::pair<theia::ViewId, int>&) { ++count[e + 1]; });
  out->match_ptr.assign(E + 1, 0);
  for (size_t e = 0; e < E; ++e) out->match_ptr[e + 1] = out->match_ptr[e] + count[e + 1];
  out->matches.assign(4 * out->match_ptr[E], 0.0);
  std::vector<uint64_t> cursor(out->match_ptr.begin(), out->match_ptr.end() - 1);
  for_each_match([&](size_t e, const std::pair<theia::ViewId, int>& lo, const std::pair<theia::ViewId, int>& hi) {
    const Eigen::Vector2d& p1 = tr.keypoints.at(lo.first)[lo.second];
    const Eigen::Vector2d& p2 = tr.keypoints.at(hi.first)[hi.second];
    double* m = &out->matches[4 * cursor[e]++];
    m[0] = p1[0]; m[1] = p1[1]; m[2] = p2[0]; m[3] = p2[1];
  });

  out->intrinsics.assign(6 * E, 0.0);
  out->rotation.assign(3 * E, 0.0);
  out->position.assign(3 * E, 0.0);
  for (size_t e = 0; e < E; ++e) {
    const theia::TwoViewInfo& info = *vg.GetEdge(out->edges[e].first, out->edges[e].second);
    const theia::ViewId v[2] = {out->edges[e].first, out->edges[e].second};
    for (int s = 0; s < 2; ++s) {
      const auto pp = tr.principal_point.find(v[s]);
      const auto fo = tr.focal.find(v[s]);
      const double u = pp == tr.principal_point.end() ? 0.0 : pp->second[0], w = pp == tr.principal_point.end() ? 0.0 : pp->second[1];
      // :99-104 reads CameraIntrinsicsPrior().focal_length, which is 0 without an EXIF entry (a singular K); the
      // median-viewing-angle guess the reader itself uses for TwoViewInfo (read_1dsfm.cc:347-357) stands in for it.
      double f = fo == tr.focal.end() ? 0.0 : fo->second;
      if (f == 0.0) f = 1.2 * u;
      out->intrinsics[6 * e + 3 * s + 0] = f;
      out->intrinsics[6 * e + 3 * s + 1] = u;
      out->intrinsics[6 * e + 3 * s + 2] = w;
    }
    for (int k = 0; k < 3; ++k) { out->rotation[3 * e + k] = info.rotation_2[k]; out->position[3 * e + k] = info.position_2[k]; }
  }
}

TrackBuildStats BuildTracksFromMatches(const EdgeMatches& em, int min_track_length, int max_track_length, Tracks1DSfM* out) {
  *out = Tracks1DSfM();
  TrackBuildStats stats;
  stats.min_track_length = min_track_length; stats.max_track_length = max_track_length;
  const size_t E = em.edges.size();
  const uint64_t M = em.match_ptr.empty() ? 0 : em.match_ptr.back();
  stats.num_matches = (size_t)M;
  // dense view index = rank of the view id; intrinsics from the first edge naming the view
  std::vector<theia::ViewId> views;
  for (const auto& e : em.edges) { views.push_back(e.first); views.push_back(e.second); }
  std::sort(views.begin(), views.end());
  views.erase(std::unique(views.begin(), views.end()), views.end());
  std::unordered_map<theia::ViewId, uint32_t> index;
  for (size_t c = 0; c < views.size(); ++c) index[views[c]] = (uint32_t)c;
  std::vector<uint32_t> edge_i(E), edge_j(E);
  for (size_t e = 0; e < E; ++e) {
    const theia::ViewId v[2] = {em.edges[e].first, em.edges[e].second};
    edge_i[e] = index.at(v[0]); edge_j[e] = index.at(v[1]);
    for (int s = 0; s < 2; ++s) {
      if (out->principal_point.count(v[s])) continue;
      const double* k = &em.intrinsics[6 * e + 3 * s];
      const auto ff = em.first_focal.find(v[s]);
      out->focal[v[s]] = ff == em.first_focal.end() ? k[0] : ff->second;
      out->principal_point[v[s]] = Eigen::Vector2d(k[1], k[2]);
    }
  }
  if (M == 0) { stats.built = true; return stats; }
  std::vector<uint64_t> track_ptr(M + 1);
  std::vector<uint32_t> obs_view(2 * M);
  std::vector<double> obs_xy(4 * M);
  gsfm_tracks_build_options o;
  gsfm_tracks_build_default_options(&o);
  o.min_track_length = min_track_length; o.max_track_length = max_track_length;
  uint64_t T = 0, O = 0;
  const gsfm_status st = gsfm_tracks_build((uint32_t)views.size(), E, edge_i.data(), edge_j.data(), em.match_ptr.data(), em.matches.data(), &o, track_ptr.data(),
                                           obs_view.data(), obs_xy.data(), &T, &O, stats.counts, &stats.kernel_ms);
  if (st == GSFM_ERR_NO_DEVICE) throw NoDeviceError(std::string("BuildTracksFromMatches: ") + gsfm_last_error());
  if (st != GSFM_OK) throw std::runtime_error(std::string("BuildTracksFromMatches: ") + gsfm_last_error());
  stats.built = true;
  stats.num_tracks = (size_t)T; stats.num_observations = (size_t)O;
  // Keypoints in feature-id order: a feature's id is the rank of its first endpoint, so walking the endpoints in the caller's order and numbering
  // a kept feature at its first hit gives each view's kept features in ascending id.  (-0.0 + 0.0 = +0.0: one key for both zeros.)
  struct Key {
    uint32_t view; uint64_t x, y;
    bool operator==(const Key& k) const { return view == k.view && x == k.x && y == k.y; }
  };
  struct KeyHash {
    size_t operator()(const Key& k) const { uint64_t h = (k.x * 0x9e3779b97f4a7c15ull) ^ (k.y + 0xbf58476d1ce4e5b9ull + (k.x << 6)); return (size_t)((h ^ (h >> 31)) * 0x94d049bb133111ebull + k.view); }
  };
  auto bits = [](double v) { v += 0.0; uint64_t b; std::memcpy(&b, &v, 8); return b; };
  std::unordered_map<Key, int, KeyHash> keypoint;   // a kept feature -> its keypoint index in its view, -1 until numbered
  keypoint.reserve((size_t)O);
  for (uint64_t k = 0; k < O; ++k) keypoint.emplace(Key{obs_view[k], bits(obs_xy[2 * k]), bits(obs_xy[2 * k + 1])}, -1);
  for (size_t e = 0; e < E; ++e)
    for (uint64_t m = em.match_ptr[e]; m < em.match_ptr[e + 1]; ++m)
      for (int s = 0; s < 2; ++s) {
        const double x = em.matches[4 * m + 2 * s], y = em.matches[4 * m + 2 * s + 1];
        const auto it = keypoint.find(Key{s ? edge_j[e] : edge_i[e], bits(x), bits(y)});
        if (it == keypoint.end() || it->second >= 0) continue;
        auto& list = out->keypoints[s ? em.edges[e].second : em.edges[e].first];
        it->second = (int)list.size();
        list.emplace_back(x, y);
      }
  out->tracks.resize((size_t)T);
  for (uint64_t t = 0; t < T; ++t)
    for (uint64_t k = track_ptr[t]; k < track_ptr[t + 1]; ++k)
      out->tracks[t].emplace_back(views[obs_view[k]], keypoint.at(Key{obs_view[k], bits(obs_xy[2 * k]), bits(obs_xy[2 * k + 1])}));
  return stats;
}

#ifndef GSFM_USE_REAL_THEIA
void FlattenTracks(const theia::Reconstruction& rec, FlatTracks* out) {
  *out = FlatTracks();
  if (!rec.tracks) return;
  const Tracks1DSfM& tr = *rec.tracks;
  for (const auto& kv : tr.keypoints) out->views.push_back(kv.first);
  std::sort(out->views.begin(), out->views.end());
  const size_t N = out->views.size();
  out->rot_aa.assign(3 * N, 0.0); out->cam_pos.assign(3 * N, 0.0); out->intrinsics.assign(3 * N, 0.0);
  out->cam_estimated.assign(N, 0);
  std::unordered_map<theia::ViewId, uint32_t> index;
  for (size_t c = 0; c < N; ++c) {
    const theia::ViewId v = out->views[c];
    index[v] = (uint32_t)c;
    const auto pp = tr.principal_point.find(v);
    const auto fo = tr.focal.find(v);
    const double u = pp == tr.principal_point.end() ? 0.0 : pp->second[0], w = pp == tr.principal_point.end() ? 0.0 : pp->second[1];
    double f = fo == tr.focal.end() ? 0.0 : fo->second;
    if (f == 0.0) f = 1.2 * u;
    const auto fe = rec.focal_length.find(v);
    if (fe != rec.focal_length.end()) f = fe->second;   // a focal length a bundle adjustment estimated
    out->intrinsics[3 * c] = f; out->intrinsics[3 * c + 1] = u; out->intrinsics[3 * c + 2] = w;
    const auto o = rec.orientation.find(v);
    const auto p = rec.position.find(v);
    if (!rec.views.count(v) || o == rec.orientation.end() || p == rec.position.end()) continue;
    out->cam_estimated[c] = 1;
    for (int k = 0; k < 3; ++k) { out->rot_aa[3 * c + k] = o->second[k]; out->cam_pos[3 * c + k] = p->second[k]; }
  }
  out->track_ptr.assign(1, 0);
  for (const auto& t : tr.tracks) {
    for (const auto& ob : t) {
      const Eigen::Vector2d& xy = tr.keypoints.at(ob.first)[ob.second];
      out->obs_cam.push_back(index.at(ob.first));
      out->obs_xy.push_back(xy[0]); out->obs_xy.push_back(xy[1]);
    }
    out->track_ptr.push_back(out->obs_cam.size());
  }
}

void KeepUnestimatedTracks(const theia::Reconstruction& rec, FlatTracks* out, std::vector<uint64_t>* track_index) {
  track_index->clear();
  std::vector<uint64_t> ptr(1, 0);
  std::vector<uint32_t> cam;
  std::vector<double> xy;
  for (size_t t = 0; t + 1 < out->track_ptr.size(); ++t) {
    if (t < rec.track_estimated.size() && rec.track_estimated[t]) continue;
    const uint64_t b = out->track_ptr[t], e = out->track_ptr[t + 1];
    cam.insert(cam.end(), out->obs_cam.begin() + b, out->obs_cam.begin() + e);
    xy.insert(xy.end(), out->obs_xy.begin() + 2 * b, out->obs_xy.begin() + 2 * e);
    ptr.push_back(cam.size());
    track_index->push_back(t);
  }
  out->track_ptr.swap(ptr); out->obs_cam.swap(cam); out->obs_xy.swap(xy);
}

EstimateStructureStats EstimateStructure(double min_angle_degrees, double max_error_pixels, theia::Reconstruction* rec, const TrackRefinement* refinement,
                                         bool only_unestimated) {
  EstimateStructureStats stats;
  gsfm_loss_node loss{};
  if (refinement) {
    const std::string& name = refinement->loss_function;
    if (name == "TRIVIAL") loss.kind = GSFM_LOSS_TRIVIAL;
    else if (name == "HUBER") loss.kind = GSFM_LOSS_HUBER;
    else if (name == "SOFTLONE") loss.kind = GSFM_LOSS_SOFT_L1;
    else throw std::runtime_error("EstimateStructure: the track refinement has no loss " + name + " (TRIVIAL, HUBER, SOFTLONE)");
    loss.p[0] = refinement->loss_width;
  }
  if (!rec->tracks || rec->tracks->tracks.empty()) return stats;   // a dataset without tracks.txt: nothing to triangulate
  FlatTracks f;
  FlattenTracks(*rec, &f);
  const size_t num_all = f.track_ptr.size() - 1;
  std::vector<uint64_t> track_index;
  if (only_unestimated) KeepUnestimatedTracks(*rec, &f, &track_index);
  const size_t T = f.track_ptr.size() - 1;
  std::vector<double> point(3 * T, 0.0);
  std::vector<int32_t> status(T, 0);
  gsfm_status st;
  if (refinement) {
    gsfm_tracks_refine_options o;
    gsfm_tracks_refine_default_options(&o);
    o.max_num_iterations = refinement->max_num_iterations;
    std::vector<int32_t> iterations(T, 0), termination(T, -1);
    uint64_t counts[7] = {0, 0, 0, 0, 0, 0, 0};
    st = gsfm_tracks_triangulate_refine((uint32_t)f.views.size(), f.rot_aa.data(), f.cam_pos.data(), f.intrinsics.data(), f.cam_estimated.data(), T,
                                        f.track_ptr.data(), f.obs_cam.data(), f.obs_xy.data(), min_angle_degrees, max_error_pixels, &o, &loss, 1,
                                        point.data(), status.data(), nullptr, nullptr, iterations.data(), nullptr, nullptr, termination.data(), counts,
                                        &stats.kernel_ms);
    for (int k = 0; k < 6; ++k) stats.counts[k] = counts[k];
    stats.tracks_refined = true;
    stats.num_refinement_failed = counts[6];
    size_t refined = 0, sum = 0;
    for (size_t t = 0; t < T; ++t)
      if (termination[t] >= 0) { ++refined; sum += (size_t)iterations[t]; stats.max_iterations = std::max(stats.max_iterations, (int)iterations[t]); }
    stats.mean_iterations = refined ? (double)sum / (double)refined : 0.0;
  } else {
    st = gsfm_tracks_triangulate((uint32_t)f.views.size(), f.rot_aa.data(), f.cam_pos.data(), f.intrinsics.data(), f.cam_estimated.data(), T,
                                 f.track_ptr.data(), f.obs_cam.data(), f.obs_xy.data(), min_angle_degrees, max_error_pixels, point.data(),
                                 status.data(), nullptr, nullptr, stats.counts, &stats.kernel_ms);
  }
  if (st != GSFM_OK) throw std::runtime_error(std::string("EstimateStructure: ") + gsfm_last_error());
  if (only_unestimated) {   // scatter by index; the estimated tracks keep point and flag
    rec->track_point.resize(num_all, Eigen::Vector3d(0.0, 0.0, 0.0));
    rec->track_estimated.resize(num_all, 0);
    for (size_t k = 0; k < T; ++k) {
      rec->track_point[track_index[k]] = Eigen::Vector3d(point[3 * k], point[3 * k + 1], point[3 * k + 2]);
      rec->track_estimated[track_index[k]] = status[k] == 0;
    }
    stats.num_tracks = T;
    stats.num_estimated = (size_t)stats.counts[0];
    return stats;
  }
  rec->track_point.assign(T, Eigen::Vector3d());
  rec->track_estimated.assign(T, 0);
  for (size_t t = 0; t < T; ++t) {
    rec->track_point[t] = Eigen::Vector3d(point[3 * t], point[3 * t + 1], point[3 * t + 2]);   // Theia leaves a rejected track's point in place too
    rec->track_estimated[t] = status[t] == 0;
  }
  stats.num_tracks = T;
  stats.num_estimated = (size_t)stats.counts[0];
  return stats;
}

UnderconstrainedStats SetUnderconstrainedAsUnestimated(theia::Reconstruction* rec) {
  UnderconstrainedStats stats;
  if (!rec->tracks) return stats;
  const auto& tracks = rec->tracks->tracks;
  auto view_estimated = [&](theia::ViewId v) { return rec->views.count(v) && rec->orientation.count(v) && rec->position.count(v); };
  auto track_estimated = [&](size_t t) { return t < rec->track_estimated.size() && rec->track_estimated[t] != 0; };
  int views = -1, removed_tracks = -1;
  while (views != 0 && removed_tracks != 0) {
    ++stats.rounds;
    // views with fewer than 3 estimated tracks (a track counts once per view, as a view's set of track ids does)
    std::unordered_map<theia::ViewId, int> seen;
    for (size_t t = 0; t < tracks.size(); ++t) {
      if (!track_estimated(t)) continue;
      std::vector<theia::ViewId> vs;
      for (const auto& ob : tracks[t]) vs.push_back(ob.first);
      std::sort(vs.begin(), vs.end());
      vs.erase(std::unique(vs.begin(), vs.end()), vs.end());
      for (theia::ViewId v : vs) ++seen[v];
    }
    std::vector<theia::ViewId> drop;
    for (theia::ViewId v : rec->views)
      if (view_estimated(v) && seen[v] < 3) drop.push_back(v);
    for (theia::ViewId v : drop) { rec->orientation.erase(v); rec->position.erase(v); }
    views = (int)drop.size();
    // tracks with fewer than 2 estimated views
    removed_tracks = 0;
    for (size_t t = 0; t < tracks.size(); ++t) {
      if (!track_estimated(t)) continue;
      std::vector<theia::ViewId> vs;
      for (const auto& ob : tracks[t]) if (view_estimated(ob.first)) vs.push_back(ob.first);
      std::sort(vs.begin(), vs.end());
      vs.erase(std::unique(vs.begin(), vs.end()), vs.end());
      if (vs.size() < 2) { rec->track_estimated[t] = 0; ++removed_tracks; }
    }
    stats.views_removed += views; stats.tracks_removed += removed_tracks;
  }
  return stats;
}

OutlierTracksStats SetOutlierTracksToUnestimated(double max_error_pixels, double min_angle_degrees, theia::Reconstruction* rec) {
  OutlierTracksStats stats;
  if (!rec->tracks || rec->tracks->tracks.empty()) return stats;
  FlatTracks f;
  FlattenTracks(*rec, &f);
  const size_t T = f.track_ptr.size() - 1;
  std::vector<uint8_t> point_estimated(T, 0);
  std::vector<double> points(3 * T, 0.0);
  for (size_t t = 0; t < T && t < rec->track_estimated.size(); ++t) {
    point_estimated[t] = rec->track_estimated[t];
    for (int k = 0; k < 3; ++k) points[3 * t + k] = rec->track_point[t][k];
  }
  std::vector<int32_t> status(T, 0);
  const gsfm_status st = gsfm_tracks_outlier_tracks((uint32_t)f.views.size(), f.rot_aa.data(), f.cam_pos.data(), f.intrinsics.data(), f.cam_estimated.data(), T,
                                                    f.track_ptr.data(), f.obs_cam.data(), f.obs_xy.data(), points.data(), point_estimated.data(),
                                                    max_error_pixels, min_angle_degrees, status.data(), nullptr, nullptr, stats.counts, &stats.kernel_ms);
  if (st != GSFM_OK) throw std::runtime_error(std::string("SetOutlierTracksToUnestimated: ") + gsfm_last_error());
  for (size_t t = 0; t < T && t < rec->track_estimated.size(); ++t)
    if (status[t] >= 2) rec->track_estimated[t] = 0;   // the point stays, as in Theia
  stats.num_examined = T - (size_t)stats.counts[1];
  stats.num_removed = (size_t)(stats.counts[2] + stats.counts[3] + stats.counts[4]);
  return stats;
}

TrackSelectionStats SelectGoodTracksForBundleAdjustment(const theia::Reconstruction& rec, int long_track_length_threshold, int image_grid_cell_size_pixels,
                                                        int min_num_optimized_tracks_per_view, std::vector<uint8_t>* tracks_to_optimize) {
  TrackSelectionStats stats;
  stats.long_track_length_threshold = long_track_length_threshold; stats.image_grid_cell_size_pixels = image_grid_cell_size_pixels;
  stats.min_num_optimized_tracks_per_view = min_num_optimized_tracks_per_view;
  tracks_to_optimize->clear();
  if (!rec.tracks || rec.tracks->tracks.empty()) return stats;
  FlatTracks f;
  FlattenTracks(rec, &f);
  const size_t T = f.track_ptr.size() - 1;
  std::vector<uint8_t> point_estimated(T, 0);
  std::vector<double> points(3 * T, 0.0);
  for (size_t t = 0; t < T && t < rec.track_estimated.size(); ++t) {
    point_estimated[t] = rec.track_estimated[t];
    for (int k = 0; k < 3; ++k) points[3 * t + k] = rec.track_point[t][k];
  }
  tracks_to_optimize->assign(T, 0);
  double top_up[2] = {0.0, 0.0};
  const gsfm_status st = gsfm_tracks_select_good((uint32_t)f.views.size(), f.rot_aa.data(), f.cam_pos.data(), f.intrinsics.data(), f.cam_estimated.data(), T,
                                                 f.track_ptr.data(), f.obs_cam.data(), f.obs_xy.data(), points.data(), point_estimated.data(),
                                                 long_track_length_threshold, image_grid_cell_size_pixels, min_num_optimized_tracks_per_view, 0,
                                                 tracks_to_optimize->data(), nullptr, nullptr, stats.counts, &stats.kernel_ms, top_up);
  if (st != GSFM_OK) throw std::runtime_error(std::string("SelectGoodTracksForBundleAdjustment: ") + gsfm_last_error());
  stats.ran = true;
  stats.num_deficient_items = (uint64_t)top_up[0]; stats.replay_ms = top_up[1];
  return stats;
}

BundleAdjustmentStats BundleAdjustCameraPositionsAndPoints(const std::string& loss_function, double loss_width, int max_num_iterations,
                                                           theia::Reconstruction* rec, const std::vector<uint8_t>* tracks_to_optimize) {
  BundleAdjustmentStats stats;
  stats.max_num_iterations = max_num_iterations;
  gsfm_loss_node loss{};
  if (loss_function == "TRIVIAL") loss.kind = GSFM_LOSS_TRIVIAL;
  else if (loss_function == "HUBER") loss.kind = GSFM_LOSS_HUBER;
  else if (loss_function == "SOFTLONE") loss.kind = GSFM_LOSS_SOFT_L1;
  else throw std::runtime_error("BundleAdjustCameraPositionsAndPoints: no loss " + loss_function + " (TRIVIAL, HUBER, SOFTLONE)");
  loss.p[0] = loss_width;
  if (!rec->tracks || rec->tracks->tracks.empty()) return stats;
  FlatTracks f;
  FlattenTracks(*rec, &f);
  const size_t T = f.track_ptr.size() - 1, N = f.views.size();
  std::vector<uint8_t> point_estimated(T, 0);
  std::vector<double> points(3 * T, 0.0);
  for (size_t t = 0; t < T && t < rec->track_estimated.size(); ++t) {
    point_estimated[t] = rec->track_estimated[t];
    for (int k = 0; k < 3; ++k) points[3 * t + k] = rec->track_point[t][k];
  }
  if (tracks_to_optimize)   // the subset: the other estimated tracks stay out of the problem and keep their points
    for (size_t t = 0; t < T; ++t) if (t >= tracks_to_optimize->size() || !(*tracks_to_optimize)[t]) point_estimated[t] = 0;
  gsfm_ba_problem* problem = nullptr;
  gsfm_status st = gsfm_ba_problem_create((uint32_t)N, f.rot_aa.data(), f.intrinsics.data(), f.cam_estimated.data(), T, f.track_ptr.data(), f.obs_cam.data(),
                                          f.obs_xy.data(), point_estimated.data(), &problem);
  if (st != GSFM_OK) throw std::runtime_error(std::string("BundleAdjustCameraPositionsAndPoints: ") + gsfm_last_error());
  gsfm_ba_options o;
  gsfm_ba_options_default(&o);
  o.max_num_iterations = max_num_iterations;
  gsfm_ba_summary s;
  st = gsfm_ba_set_loss(problem, &loss, 1);
  if (st == GSFM_OK) st = gsfm_ba_solve(problem, f.cam_pos.data(), points.data(), &o, &s);
  gsfm_ba_problem_destroy(problem);
  if (st != GSFM_OK) throw std::runtime_error(std::string("BundleAdjustCameraPositionsAndPoints: ") + gsfm_last_error());
  for (size_t c = 0; c < N; ++c)
    if (f.cam_estimated[c]) rec->position[f.views[c]] = Eigen::Vector3d(f.cam_pos[3 * c], f.cam_pos[3 * c + 1], f.cam_pos[3 * c + 2]);
  for (size_t t = 0; t < T; ++t)
    if (point_estimated[t]) rec->track_point[t] = Eigen::Vector3d(points[3 * t], points[3 * t + 1], points[3 * t + 2]);
  stats.ran = true;
  stats.usable = s.termination != GSFM_TERM_FAILURE;
  stats.termination = s.termination; stats.num_iterations = s.num_iterations; stats.num_successful_steps = s.num_successful_steps;
  stats.num_unsuccessful_steps = s.num_unsuccessful_steps; stats.num_cg_iterations = s.num_cg_iterations;
  stats.num_observations = s.num_observations_used; stats.num_cameras = s.num_active_cameras; stats.num_points = s.num_active_points;
  stats.initial_cost = s.initial_cost; stats.final_cost = s.final_cost; stats.t_total_ms = s.t_total_ms;
  return stats;
}

namespace {
const struct { const char* name; int bit; } kIntrinsicsBits[] = {
    {"FOCAL_LENGTH", (int)OptimizeIntrinsicsType::FOCAL_LENGTH}, {"ASPECT_RATIO", (int)OptimizeIntrinsicsType::ASPECT_RATIO}, {"SKEW", (int)OptimizeIntrinsicsType::SKEW},
    {"PRINCIPAL_POINTS", (int)OptimizeIntrinsicsType::PRINCIPAL_POINTS}, {"RADIAL_DISTORTION", (int)OptimizeIntrinsicsType::RADIAL_DISTORTION},
    {"TANGENTIAL_DISTORTION", (int)OptimizeIntrinsicsType::TANGENTIAL_DISTORTION}};
}  // namespace

bool ParseOptimizeIntrinsicsType(const std::string& text, int* mask, std::string* error) {
  *mask = (int)OptimizeIntrinsicsType::NONE;
  if (text.empty()) { if (error) *error = "intrinsics_to_optimize is empty (NONE, ALL, or names joined by '|')"; return false; }
  std::stringstream ss(text);
  std::string item;
  bool first = true;
  int m = 0;
  while (std::getline(ss, item, '|')) {
    if (first && item == "NONE") return true;
    if (first && item == "ALL") { *mask = (int)OptimizeIntrinsicsType::ALL; return true; }
    first = false;
    int bit = 0;
    for (const auto& b : kIntrinsicsBits) if (item == b.name) bit = b.bit;
    if (!bit) { if (error) *error = "intrinsics_to_optimize: no intrinsic parameter named '" + item + "'"; return false; }
    m |= bit;
  }
  *mask = m;
  return true;
}

std::string OptimizeIntrinsicsTypeNames(int mask) {
  std::string out;
  for (const auto& b : kIntrinsicsBits) if (mask & b.bit) out += (out.empty() ? "" : "|") + std::string(b.name);
  return out.empty() ? "NONE" : out;
}

BundleAdjustmentStats BundleAdjustment(const std::string& loss_function, double loss_width, int max_num_iterations, int intrinsics_to_optimize,
                                       theia::Reconstruction* rec, const std::vector<uint8_t>* tracks_to_optimize) {
  BundleAdjustmentStats stats;
  stats.max_num_iterations = max_num_iterations;
  const int unsupported = intrinsics_to_optimize & ~(int)OptimizeIntrinsicsType::FOCAL_LENGTH;
  if (unsupported)   // holding what the caller asked to move, without a word, is not an option
    throw std::invalid_argument("BundleAdjustment: intrinsics_to_optimize asks for " + OptimizeIntrinsicsTypeNames(unsupported) +
                                ", which the device bundle adjustment does not optimise (supported: NONE, FOCAL_LENGTH)");
  const bool focal = intrinsics_to_optimize == (int)OptimizeIntrinsicsType::FOCAL_LENGTH;
  gsfm_loss_node loss{};
  if (loss_function == "TRIVIAL") loss.kind = GSFM_LOSS_TRIVIAL;
  else if (loss_function == "HUBER") loss.kind = GSFM_LOSS_HUBER;
  else if (loss_function == "SOFTLONE") loss.kind = GSFM_LOSS_SOFT_L1;
  else throw std::runtime_error("BundleAdjustment: no loss " + loss_function + " (TRIVIAL, HUBER, SOFTLONE)");
  loss.p[0] = loss_width;
  if (!rec->tracks || rec->tracks->tracks.empty()) return stats;
  FlatTracks f;
  FlattenTracks(*rec, &f);
  const size_t T = f.track_ptr.size() - 1, N = f.views.size();
  std::vector<uint8_t> point_estimated(T, 0);
  std::vector<double> points(3 * T, 0.0);
  for (size_t t = 0; t < T && t < rec->track_estimated.size(); ++t) {
    point_estimated[t] = rec->track_estimated[t];
    for (int k = 0; k < 3; ++k) points[3 * t + k] = rec->track_point[t][k];
  }
  if (tracks_to_optimize)   // the subset: the other estimated tracks stay out of the problem and keep their points
    for (size_t t = 0; t < T; ++t) if (t >= tracks_to_optimize->size() || !(*tracks_to_optimize)[t]) point_estimated[t] = 0;
  gsfm_ba_options o;
  gsfm_ba_summary s;
  gsfm_status st;
  std::vector<double> focal_length(N, 0.0);
  if (focal) {
    for (size_t c = 0; c < N; ++c) focal_length[c] = f.intrinsics[3 * c];
    gsfm_ba7_problem* problem = nullptr;
    st = gsfm_ba7_problem_create((uint32_t)N, f.intrinsics.data(), f.cam_estimated.data(), nullptr, T, f.track_ptr.data(), f.obs_cam.data(), f.obs_xy.data(),
                                 point_estimated.data(), &problem);
    if (st != GSFM_OK) throw std::runtime_error(std::string("BundleAdjustment: ") + gsfm_last_error());
    gsfm_ba7_options_default(&o);
    o.max_num_iterations = max_num_iterations;
    st = gsfm_ba7_set_loss(problem, &loss, 1);
    if (st == GSFM_OK) st = gsfm_ba7_solve(problem, f.rot_aa.data(), f.cam_pos.data(), focal_length.data(), points.data(), &o, &s);
    gsfm_ba7_problem_destroy(problem);
  } else {
    gsfm_ba6_problem* problem = nullptr;
    st = gsfm_ba6_problem_create((uint32_t)N, f.intrinsics.data(), f.cam_estimated.data(), T, f.track_ptr.data(), f.obs_cam.data(), f.obs_xy.data(),
                                 point_estimated.data(), &problem);
    if (st != GSFM_OK) throw std::runtime_error(std::string("BundleAdjustment: ") + gsfm_last_error());
    gsfm_ba6_options_default(&o);
    o.max_num_iterations = max_num_iterations;
    st = gsfm_ba6_set_loss(problem, &loss, 1);
    if (st == GSFM_OK) st = gsfm_ba6_solve(problem, f.rot_aa.data(), f.cam_pos.data(), points.data(), &o, &s);
    gsfm_ba6_problem_destroy(problem);
  }
  if (st != GSFM_OK) throw std::runtime_error(std::string("BundleAdjustment: ") + gsfm_last_error());
  for (size_t c = 0; c < N; ++c)
    if (f.cam_estimated[c]) {
      rec->orientation[f.views[c]] = Eigen::Vector3d(f.rot_aa[3 * c], f.rot_aa[3 * c + 1], f.rot_aa[3 * c + 2]);
      rec->position[f.views[c]] = Eigen::Vector3d(f.cam_pos[3 * c], f.cam_pos[3 * c + 1], f.cam_pos[3 * c + 2]);
      if (focal) rec->focal_length[f.views[c]] = focal_length[c];
    }
  for (size_t t = 0; t < T; ++t)
    if (point_estimated[t]) rec->track_point[t] = Eigen::Vector3d(points[3 * t], points[3 * t + 1], points[3 * t + 2]);
  stats.ran = true;
  stats.focal_lengths_free = focal;
  stats.usable = s.termination != GSFM_TERM_FAILURE;
  stats.termination = s.termination; stats.num_iterations = s.num_iterations; stats.num_successful_steps = s.num_successful_steps;
  stats.num_unsuccessful_steps = s.num_unsuccessful_steps; stats.num_cg_iterations = s.num_cg_iterations;
  stats.num_observations = s.num_observations_used; stats.num_cameras = s.num_active_cameras; stats.num_points = s.num_active_points;
  stats.initial_cost = s.initial_cost; stats.final_cost = s.final_cost; stats.t_total_ms = s.t_total_ms;
  return stats;
}

bool WritePlyFile(const std::string& ply_file, const theia::Reconstruction& rec, int min_num_observations_per_point) {
  std::ofstream f(ply_file);
  if (!f.is_open()) return false;
  std::vector<size_t> tracks;
  for (size_t t = 0; t < rec.track_estimated.size(); ++t)
    if (rec.track_estimated[t] && rec.tracks && (int)rec.tracks->tracks[t].size() >= min_num_observations_per_point) tracks.push_back(t);
  size_t n = tracks.size();
  for (const auto& kv : rec.orientation) n += rec.views.count(kv.first);
  f << "ply\nformat ascii 1.0\nelement vertex " << n
    << "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header" << std::endl;
  for (size_t t : tracks) f << rec.track_point[t][0] << " " << rec.track_point[t][1] << " " << rec.track_point[t][2] << " 0 0 0\n";
  for (const auto& kv : rec.orientation) {
    if (!rec.views.count(kv.first)) continue;
    auto it = rec.position.find(kv.first);
    if (it == rec.position.end()) f << "0 0 0 0 255 0\n";
    else f << it->second[0] << " " << it->second[1] << " " << it->second[2] << " 0 255 0\n";
  }
  return (bool)f;
}
#endif

bool StoreCovarianceRot(const std::string& dir, const EdgeMatches& all, const theia::ViewGraph& vg, CovarianceMap* cov_out,
                        CalcCovarianceStats* stats, std::string* error) {
  // keep the pairs that are (still) edges of the view graph; rotation_2 / position_2 come from the graph's TwoViewInfo
  EdgeMatches em;
  em.match_ptr.push_back(0);
  for (size_t e = 0; e < all.edges.size(); ++e) {
    const theia::TwoViewInfo* info = vg.GetEdge(all.edges[e].first, all.edges[e].second);
    if (!info) continue;
    em.edges.push_back(all.edges[e]);
    em.matches.insert(em.matches.end(), all.matches.begin() + 4 * all.match_ptr[e], all.matches.begin() + 4 * all.match_ptr[e + 1]);
    em.match_ptr.push_back(em.matches.size() / 4);
    em.intrinsics.insert(em.intrinsics.end(), all.intrinsics.begin() + 6 * e, all.intrinsics.begin() + 6 * e + 6);
    for (int k = 0; k < 3; ++k) { em.rotation.push_back(info->rotation_2[k]); em.position.push_back(info->position_2[k]); }
  }
  const size_t E = em.edges.size();
  std::vector<double> cov9(9 * E), rot(3 * E), trans(3 * E);
  std::vector<int32_t> status(E), iters(E);
  double kernel_ms = 0.0;
  if (E > 0) {
    // 500 iterations: the reference's hard-coded Solver::Options (src/uncertainty.cpp:141-146)
    const gsfm_status st = gsfm_cov_estimate(E, em.match_ptr.data(), em.matches.data(), em.intrinsics.data(), em.rotation.data(), em.position.data(),
                                             500, cov9.data(), rot.data(), trans.data(), status.data(), iters.data(), &kernel_ms);
    if (st != GSFM_OK) { if (error) *error = gsfm_last_error(); return false; }
  }
  CovarianceMap result;
  CalcCovarianceStats s;
  s.num_edges = E;
  s.num_matches = em.match_ptr.back();
  s.kernel_ms = kernel_ms;
  for (size_t e = 0; e < E; ++e) {
    if (status[e] == 1) { ++s.num_skipped; continue; }
    if (status[e] != 0) { ++s.num_singular; continue; }
    Eigen::Matrix3d C;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C(r, c) = cov9[9 * e + 3 * r + c];
    result[em.edges[e]] = std::make_pair(C, Eigen::Vector3d(rot[3 * e], rot[3 * e + 1], rot[3 * e + 2]));
    ++s.num_written;
  }
  if (!WriteCovariance(dir, result)) { if (error) *error = "cannot write " + dir + "/covariance_rot.txt"; return false; }
  if (cov_out) *cov_out = std::move(result);
  if (stats) *stats = s;
  return true;
}

bool CalcCovariance(const std::string& dir, CovarianceMap* cov_out, CalcCovarianceStats* stats, std::string* error) {
  Tracks1DSfM tracks;
  if (!Read1DSFMTracks(dir, &tracks, error)) return false;
  theia::ViewGraph vg;
  if (!Read1DSFMViewGraph(dir, &vg, error)) return false;
  EdgeMatches em;
  CollectEdgeMatches(tracks, vg, &em);
  return StoreCovarianceRot(dir, em, vg, cov_out, stats, error);
}

// ------------------------------------------------------------------------------------------------------------------
// COLMAP export (two_views.txt)
// ------------------------------------------------------------------------------------------------------------------
bool ReadImageSize(const std::string& path, int* width, int* height) {
  std::ifstream f(path, std::ios::binary);
  if (!f.is_open()) return false;
  unsigned char h[26];
  f.read((char*)h, 24);
  if (f.gcount() >= 24 && h[0] == 0x89 && h[1] == 'P' && h[2] == 'N' && h[3] == 'G') {  // PNG: IHDR follows the 8-byte signature
    *width = (h[16] << 24) | (h[17] << 16) | (h[18] << 8) | h[19];
    *height = (h[20] << 24) | (h[21] << 16) | (h[22] << 8) | h[23];
    return true;
  }
  if (f.gcount() < 4 || h[0] != 0xFF || h[1] != 0xD8) return false;
  f.clear();
  f.seekg(2);
  for (;;) {  // JPEG: walk the marker segments to the first start-of-frame
    int c = f.get();
    if (c == EOF) return false;
    if (c != 0xFF) continue;
    int m = f.get();
    while (m == 0xFF) m = f.get();
    if (m == EOF) return false;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;  // markers without a length
    unsigned char l[2];
    if (!f.read((char*)l, 2)) return false;
    const int len = (l[0] << 8) | l[1];
    const bool sof = m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC;
    if (sof) {
      unsigned char d[5];
      if (!f.read((char*)d, 5)) return false;
      *height = (d[1] << 8) | d[2];
      *width = (d[3] << 8) | d[4];
      return true;
    }
    f.seekg(len - 2, std::ios::cur);
  }
}

bool ReadColmapTwoViews(const std::string& path, const std::vector<std::string>& image_paths, ColmapPoseGraph* out, std::string* error) {
  *out = ColmapPoseGraph();
  std::unordered_map<std::string, Eigen::Vector2d> pp_by_name;
  for (const std::string& ip : image_paths) {
    int w = 0, h = 0;
    if (!ReadImageSize(ip, &w, &h)) { if (error) *error = "cannot read the size of image " + ip; return false; }
    const size_t slash = ip.find_last_of('/');
    pp_by_name[slash == std::string::npos ? ip : ip.substr(slash + 1)] = Eigen::Vector2d(w / 2, h / 2);  // integer halves, :80-82
  }
  std::ifstream fin(path);
  if (!fin.is_open()) { if (error) *error = "cannot read " + path; return false; }
  std::string line;
  for (int k = 0; k < 3; ++k) std::getline(fin, line);
  std::unordered_map<std::string, theia::ViewId> id_of;
  auto view_id = [&](const std::string& name) {
    auto it = id_of.find(name);
    if (it != id_of.end()) return it->second;
    const theia::ViewId id = (theia::ViewId)out->view_names.size();
    id_of[name] = id;
    out->view_names.push_back(name);
    const auto pp = pp_by_name.find(name);
    out->principal_point[id] = pp == pp_by_name.end() ? Eigen::Vector2d(0, 0) : pp->second;  // unknown image: operator[] default (:117-120)
    return id;
  };
  struct Pair { theia::ViewIdPair key; std::vector<double> m; double intr[6]; };
  std::vector<Pair> pairs;
  std::string n1, n2;
  double f1, f2, r[3], t[3];
  long num = 0;
  while (fin >> n1 >> n2 >> f1 >> f2 >> num >> r[0] >> r[1] >> r[2] >> t[0] >> t[1] >> t[2]) {
    if (num < 0) { if (error) *error = "negative inlier count in " + path; return false; }
    std::vector<double> a(2 * num), b(2 * num);
    for (double& v : a) if (!(fin >> v)) { if (error) *error = "two_views.txt ends inside a feature list"; return false; }
    for (double& v : b) if (!(fin >> v)) { if (error) *error = "two_views.txt ends inside a feature list"; return false; }
    theia::ViewId i = view_id(n1), j = view_id(n2);
    if (i == j) continue;
    out->matches.first_focal.emplace(i, f1);   // (emplace keeps the first line's value)
    out->matches.first_focal.emplace(j, f2);
    theia::TwoViewInfo info;
    info.focal_length_1 = f1; info.focal_length_2 = f2;
    info.num_homography_inliers = info.num_verified_matches = info.visibility_score = (int)num;
    info.rotation_2 = Eigen::Vector3d(r[0], r[1], r[2]);
    info.position_2 = Eigen::Vector3d(t[0], t[1], t[2]);
    if (i > j) {  // SwapCameras: focal lengths swap, position <- -(R * position), rotation <- -rotation
      std::swap(info.focal_length_1, info.focal_length_2);
      double R[9], q[3];
      AngleAxisToRowMajorMatrix(info.rotation_2.data(), R);
      for (int a3 = 0; a3 < 3; ++a3) q[a3] = -(R[3 * a3] * t[0] + R[3 * a3 + 1] * t[1] + R[3 * a3 + 2] * t[2]);
      info.position_2 = Eigen::Vector3d(q[0], q[1], q[2]);
      info.rotation_2 = Eigen::Vector3d(-r[0], -r[1], -r[2]);
      std::swap(i, j);
      a.swap(b);
    }
    out->view_graph.AddEdge(i, j, info);
    Pair p;
    p.key = theia::ViewIdPair(i, j);
    p.m.resize(4 * num);
    for (long k = 0; k < num; ++k) { p.m[4 * k] = a[2 * k]; p.m[4 * k + 1] = a[2 * k + 1]; p.m[4 * k + 2] = b[2 * k]; p.m[4 * k + 3] = b[2 * k + 1]; }
    const Eigen::Vector2d &pi = out->principal_point[i], &pj = out->principal_point[j];
    const double intr[6] = {info.focal_length_1, pi[0], pi[1], info.focal_length_2, pj[0], pj[1]};
    std::memcpy(p.intr, intr, sizeof(intr));
    pairs.push_back(std::move(p));
  }
  // a pair listed twice: the later row wins, as AddEdge overwrites
  std::stable_sort(pairs.begin(), pairs.end(), [](const Pair& x, const Pair& y) { return x.key < y.key; });
  EdgeMatches& em = out->matches;
  em.match_ptr.push_back(0);
  for (size_t k = 0; k < pairs.size(); ++k) {
    if (k + 1 < pairs.size() && pairs[k + 1].key == pairs[k].key) continue;
    const theia::TwoViewInfo& info = *out->view_graph.GetEdge(pairs[k].key.first, pairs[k].key.second);
    em.edges.push_back(pairs[k].key);
    em.matches.insert(em.matches.end(), pairs[k].m.begin(), pairs[k].m.end());
    em.match_ptr.push_back(em.matches.size() / 4);
    em.intrinsics.insert(em.intrinsics.end(), pairs[k].intr, pairs[k].intr + 6);
    for (int c = 0; c < 3; ++c) { em.rotation.push_back(info.rotation_2[c]); em.position.push_back(info.position_2[c]); }
  }
  return true;
}

std::vector<std::string> ExpandWildcard(const std::string& pattern) {
  std::vector<std::string> out;
  glob_t g;
  if (glob(pattern.c_str(), 0, nullptr, &g) == 0) {
    for (size_t k = 0; k < g.gl_pathc; ++k) out.emplace_back(g.gl_pathv[k]);
  }
  globfree(&g);
  return out;
}

}  // namespace gsfm

#ifndef GSFM_USE_REAL_THEIA
namespace theia {
int Reconstruction::NumTracks() const { return tracks ? (int)tracks->tracks.size() : 0; }
int Reconstruction::NumEstimatedTracks() const { return (int)std::count(track_estimated.begin(), track_estimated.end(), (uint8_t)1); }
}  // namespace theia
#endif
