// lslam_adapters.hpp -- header-only C++ host layer above the C ABI (include/lslam_gpu.h).
//
// The reference's seams for this path are C++ classes, not an FFI; these two
// adapters mirror their names, argument meaning and error behaviour so a maintainer of the
// reference can swap call sites one for one:
//   lslam::GpuScanMatcher  <-> karto::ScanMatcher                 (Mapper.h:1127-1279)
//   lslam::MapRepGpu       <-> hectorslam::MapRepresentationInterface (H/slam_main/
//                              MapRepresentationInterface.h:44-69), update side
//   lslam::GpuScanMatcherMap <-> gmapping::ScanMatcherMap        (lesson4/include/lesson4/gmapping/grid/map.h),
//                              read side + the lesson4 GMapping node's ComputeMap
// Only PODs appear here so the header builds without open_karto / Eigen; INTEGRATION.md shows the
// few lines that convert karto::LocalizedRangeScan / hectorslam::DataContainer to these PODs.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "lslam_gpu.h"

namespace lslam {

struct Pose2 {  // karto::Pose2 (Karto.h:1959-2168): x, y, heading
  double x = 0, y = 0, heading = 0;
};
struct Matrix3 {  // karto::Matrix3 (Karto.h:2344-2613), row-major
  double m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  double& operator()(int r, int c) { return m[r][c]; }
  double operator()(int r, int c) const { return m[r][c]; }
};
// what MatchScan reads from a karto::LocalizedRangeScan: GetRangeReadings() + GetSensorPose()
struct RangeScan {
  const double* ranges = nullptr;  // >= num_beams readings
  Pose2 sensor_pose;
};

// the exceptions the reference throws on this path (Mapper.cpp:444-447,484-487; Karto.h:4488-4499)
struct MatcherError : std::runtime_error {
  int status;
  MatcherError(int s, const std::string& w) : std::runtime_error(w), status(s) {}
};

class GpuScanMatcher {
 public:
  // ScanMatcher::Create (Mapper.h:1139-1143): nullptr on invalid parameters, throws
  // std::runtime_error for a bad smear deviation (Mapper.h:1041-1053)
  static GpuScanMatcher* Create(lslam_context* ctx, const lslam_matcher_config& cfg, const lslam_laser& laser) {
    lslam_matcher* h = nullptr;
    int rc = lslam_matcher_create(ctx, &cfg, &laser, &h);
    if (rc == LSLAM_ERR_INVALID_ARGUMENT) return nullptr;
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx));
    return new GpuScanMatcher(ctx, h, laser);
  }
  ~GpuScanMatcher() { lslam_matcher_destroy(h_); }
  GpuScanMatcher(const GpuScanMatcher&) = delete;
  GpuScanMatcher& operator=(const GpuScanMatcher&) = delete;

  // kt_double MatchScan(pScan, rBaseScans, rMean, rCovariance, doPenalize, doRefineMatch)
  // (Mapper.h:1155-1159)
  double MatchScan(const RangeScan& scan, const std::vector<RangeScan>& baseScans, Pose2& rMean,
                   Matrix3& rCovariance, bool doPenalize = true, bool doRefineMatch = true) {
    const int n = lslam_matcher_num_beams(h_);
    const int stride = n > 0 ? n : 1;
    ranges_.resize(baseScans.size() * (size_t)stride);
    poses_.resize(baseScans.size() * 3);
    for (size_t i = 0; i < baseScans.size(); i++) {
      std::memcpy(&ranges_[i * stride], baseScans[i].ranges, sizeof(double) * (size_t)n);
      poses_[3 * i] = baseScans[i].sensor_pose.x;
      poses_[3 * i + 1] = baseScans[i].sensor_pose.y;
      poses_[3 * i + 2] = baseScans[i].sensor_pose.heading;
    }
    const double q[3] = {scan.sensor_pose.x, scan.sensor_pose.y, scan.sensor_pose.heading};
    lslam_match_result r;
    check(lslam_matcher_match_scan(h_, (int)baseScans.size(), ranges_.data(), stride, poses_.data(), scan.ranges, q,
                                   doPenalize, doRefineMatch, &r));
    return unpack(r, rMean, rCovariance);
  }

  // AddScans (Mapper.cpp:699-708) around an explicit centre + the search against the current
  // grid for many independent scans (the batched mode; no equivalent single call in the reference)
  void AddScans(const std::vector<RangeScan>& baseScans, const Pose2& center) {
    const int n = lslam_matcher_num_beams(h_);
    const int stride = n > 0 ? n : 1;
    ranges_.resize(baseScans.size() * (size_t)stride);
    poses_.resize(baseScans.size() * 3);
    for (size_t i = 0; i < baseScans.size(); i++) {
      std::memcpy(&ranges_[i * stride], baseScans[i].ranges, sizeof(double) * (size_t)n);
      poses_[3 * i] = baseScans[i].sensor_pose.x;
      poses_[3 * i + 1] = baseScans[i].sensor_pose.y;
      poses_[3 * i + 2] = baseScans[i].sensor_pose.heading;
    }
    const double c[3] = {center.x, center.y, center.heading};
    check(lslam_matcher_set_base_scans(h_, (int)baseScans.size(), ranges_.data(), stride, poses_.data(), c));
  }
  std::vector<lslam_match_result> MatchBatch(const std::vector<RangeScan>& scans, bool doPenalize = true,
                                             bool doRefineMatch = true) {
    const int n = lslam_matcher_num_beams(h_);
    const int stride = n > 0 ? n : 1;
    ranges_.resize(scans.size() * (size_t)stride);
    poses_.resize(scans.size() * 3);
    for (size_t i = 0; i < scans.size(); i++) {
      std::memcpy(&ranges_[i * stride], scans[i].ranges, sizeof(double) * (size_t)n);
      poses_[3 * i] = scans[i].sensor_pose.x;
      poses_[3 * i + 1] = scans[i].sensor_pose.y;
      poses_[3 * i + 2] = scans[i].sensor_pose.heading;
    }
    std::vector<lslam_match_result> out(scans.size());
    check(lslam_matcher_match_batch(h_, (int)scans.size(), ranges_.data(), stride, poses_.data(), doPenalize,
                                    doRefineMatch, out.data()));
    return out;
  }

  // MatchBatch as `depth` pipelined sub-batches (LSLAM_OPT_PIPELINE_DEPTH, 1..4; lslam_gpu.h): the upload of one
  // runs under the kernels of the other, their response kernels fill each other's tails.  Same records.  No reference counterpart.
  void SetPipelineDepth(int depth) { check(lslam_matcher_set_option(h_, LSLAM_OPT_PIPELINE_DEPTH, depth)); }

  // LocalizedRangeScan::GetSensorAt / SetSensorPose (Karto.h:5280-5313)
  Pose2 SensorPoseFromRobot(const Pose2& robot) const {
    const double r[3] = {robot.x, robot.y, robot.heading};
    double s[3];
    lslam_sensor_pose_from_robot(&laser_, r, s);
    return Pose2{s[0], s[1], s[2]};
  }
  Pose2 RobotPoseFromSensor(const Pose2& sensor) const {
    const double s[3] = {sensor.x, sensor.y, sensor.heading};
    double r[3];
    lslam_robot_pose_from_sensor(&laser_, s, r);
    return Pose2{r[0], r[1], r[2]};
  }
  lslam_matcher* handle() { return h_; }

 private:
  GpuScanMatcher(lslam_context* ctx, lslam_matcher* h, const lslam_laser& laser) : ctx_(ctx), h_(h), laser_(laser) {}
  void check(int rc) {
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
  }
  static double unpack(const lslam_match_result& r, Pose2& mean, Matrix3& cov) {
    if (r.status != LSLAM_OK) throw MatcherError(r.status, "scan matcher: the reference throws here");
    mean = Pose2{r.pose[0], r.pose[1], r.pose[2]};
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) cov.m[i][j] = r.covariance[3 * i + j];
    return r.response;
  }
  lslam_context* ctx_;
  lslam_matcher* h_;
  lslam_laser laser_;
  std::vector<double> ranges_, poses_;
};

// Pose path of karto::Mapper::Process (Mapper.cpp:1999-2079) with a device-resident running-scan
// window: what SlamKarto::addScan calls per LaserScan (karto_slam.cc:444).  The pose graph
// (vertices, edges, loop closure) stays with the reference's host code.
class GpuFrontEnd {
 public:
  // scanBufferSize / scanBufferMaximumScanDistance / minimumTravelDistance / minimumTravelHeading:
  // the Mapper parameters of the same names (Mapper.cpp:1480-1515)
  GpuFrontEnd(lslam_context* ctx, GpuScanMatcher& matcher, int scanBufferSize, double scanBufferMaximumScanDistance,
              double minimumTravelDistance, double minimumTravelHeading)
      : ctx_(ctx) {
    int rc = lslam_frontend_create(matcher.handle(), scanBufferSize, scanBufferMaximumScanDistance,
                                   minimumTravelDistance, minimumTravelHeading, &h_);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx));
  }
  ~GpuFrontEnd() { lslam_frontend_destroy(h_); }
  GpuFrontEnd(const GpuFrontEnd&) = delete;
  GpuFrontEnd& operator=(const GpuFrontEnd&) = delete;

  // kt_bool Process(LocalizedRangeScan*): ranges + odometric robot pose in; returns whether the scan
  // was processed (HasMovedEnough) and its corrected robot pose (GetCorrectedPose) / covariance
  bool Process(const double* ranges, int nRanges, const Pose2& odometricPose, Pose2& correctedPose,
               Matrix3* covariance = nullptr, double* response = nullptr) {
    const double o[3] = {odometricPose.x, odometricPose.y, odometricPose.heading};
    double c[3], cov[9];
    int processed = 0;
    int rc = lslam_frontend_process(h_, ranges, nRanges, o, &processed, c, cov, response);
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
    correctedPose = Pose2{c[0], c[1], c[2]};
    if (covariance && processed)
      for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) covariance->m[i][j] = cov[3 * i + j];
    return processed != 0;
  }
  // Process for a recorded trajectory (nScans scans already at hand, rows of rangesStride doubles, poses as x, y, heading
  // triples): one scan of look-ahead, same results (lslam_frontend_process_many).  processed[i] / corrected[3 i ..] as Process.
  void ProcessMany(const double* ranges, int rangesStride, const double* odometricPoses, int nScans, std::vector<int32_t>& processed,
                   std::vector<double>& corrected) {
    processed.assign((size_t)nScans, 0);
    corrected.assign((size_t)nScans * 3, 0.0);
    int rc = lslam_frontend_process_many(h_, nScans, ranges, rangesStride, odometricPoses, nullptr, processed.data(), corrected.data(),
                                         nullptr, nullptr);
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
  }
  int RunningScans() const { return lslam_frontend_running_scans(h_); }
  lslam_frontend* handle() const { return h_; }
  lslam_context* context() const { return ctx_; }

 private:
  lslam_context* ctx_;
  lslam_frontend* h_ = nullptr;
};

// The map SlamKarto::updateMap publishes (karto_slam.cc:507-581): OccupancyGrid::CreateFromScans(
// mapper_->GetAllProcessedScans(), resolution_) over the front-end's resident scans, kept up to date on the device
// (lslam_livemap_*).  Update() replaces the CreateFromScans call; GetWidth / GetHeight / GetOffset and ReadRos are what
// the callback reads afterwards (:527-569).  Declare it after the front-end it reads: it must be destroyed first.
class LiveOccupancyGrid {
 public:
  LiveOccupancyGrid(GpuFrontEnd& frontEnd, double resolution) : ctx_(frontEnd.context()) {
    int rc = lslam_frontend_livemap_create(frontEnd.handle(), resolution, &h_);
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
  }
  ~LiveOccupancyGrid() { lslam_livemap_destroy(h_); }
  LiveOccupancyGrid(const LiveOccupancyGrid&) = delete;
  LiveOccupancyGrid& operator=(const LiveOccupancyGrid&) = delete;

  // false where the reference's CreateFromScans returns NULL (no processed scan yet: updateMap returns false, :514-515)
  bool Update() {
    int rc = lslam_livemap_update(h_);
    if (rc == LSLAM_ERR_INVALID_ARGUMENT) return false;
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
    Info();
    return true;
  }
  int GetWidth() const { return dims_[0]; }
  int GetHeight() const { return dims_[1]; }
  // GetCoordinateConverter()->GetOffset()
  void GetOffset(double& x, double& y) const { x = off_[0]; y = off_[1]; }
  // nav_msgs/OccupancyGrid data as karto_slam.cc:546-569 fills it (-1 unknown, 100 occupied, 0 free), width * height
  void ReadRos(int8_t* data) {
    int rc = lslam_occgrid_read_ros_i8(Grid(), data);
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
  }
  // GetValue(x, y) for every cell: GridStates (Karto.h:4193-4198)
  void Read(uint8_t* data) {
    int rc = lslam_occgrid_read_u8(Grid(), data);
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
  }
  // borrowed: valid until the next Update
  lslam_occgrid* Grid() { return lslam_livemap_grid(h_); }
  // updates, appends, grows, rebuilds, scans traced (all updates), scans in the map
  std::vector<int64_t> Stats() const {
    std::vector<int64_t> s(6, 0);
    lslam_livemap_stats(h_, s.data());
    return s;
  }

 private:
  void Info() {
    double res = 0.0;
    lslam_occgrid_info(Grid(), dims_, off_, &res);
  }
  lslam_context* ctx_;
  lslam_livemap* h_ = nullptr;
  int32_t dims_[2] = {0, 0};
  double off_[2] = {0.0, 0.0};
};

// karto::OccupancyGrid::RayCast (Karto.h:5717-5755) over a map that lives on the device: the distance from a pose along
// its heading to the first cell that is not free, at most maxRange.  Borrows an lslam_occgrid -- one built by
// lslam_occgrid_create_* or the live map's (LiveOccupancyGrid::Grid(), valid until its next Update) -- and never
// releases it.  RayCast is the reference's call with plain doubles; RayCastMany and RayCastScans are what a localiser or
// a scan synthesiser wants: many rays, or whole range images, per call.
class OccupancyGridRayCaster {
 public:
  OccupancyGridRayCaster(lslam_context* ctx, lslam_occgrid* grid) : ctx_(ctx), og_(grid) {}

  // RayCast(Pose2(x, y, heading), maxRange)
  double RayCast(double x, double y, double heading, double maxRange) const {
    const double pose[3] = {x, y, heading};
    double d = 0.0;
    Check(lslam_occgrid_ray_cast(og_, 1, pose, nullptr, maxRange, &d));
    return d;
  }
  // poses: (x, y, heading) per ray; one maxRange for all of them
  std::vector<double> RayCastMany(const std::vector<Pose2>& poses, double maxRange) const {
    std::vector<double> xyh(poses.size() * 3), out(poses.size());
    for (size_t i = 0; i < poses.size(); i++) { xyh[3 * i] = poses[i].x; xyh[3 * i + 1] = poses[i].y; xyh[3 * i + 2] = poses[i].heading; }
    Check(lslam_occgrid_ray_cast(og_, static_cast<int>(poses.size()), xyh.data(), nullptr, maxRange, out.data()));
    return out;
  }
  // ... or one per ray
  std::vector<double> RayCastMany(const std::vector<Pose2>& poses, const std::vector<double>& maxRanges) const {
    if (maxRanges.size() != poses.size()) throw std::invalid_argument("lslam: one max range per ray");
    std::vector<double> xyh(poses.size() * 3), out(poses.size());
    for (size_t i = 0; i < poses.size(); i++) { xyh[3 * i] = poses[i].x; xyh[3 * i + 1] = poses[i].y; xyh[3 * i + 2] = poses[i].heading; }
    Check(lslam_occgrid_ray_cast(og_, static_cast<int>(poses.size()), xyh.data(), maxRanges.data(), 0.0, out.data()));
    return out;
  }
  // The range image `laser` sees from every SENSOR pose: beam i looks along heading + minimum_angle + i * angular_resolution
  // (Karto.h:5394).  Row-major [poses][numBeams] -- the `ranges` layout GpuScanMatcher and GpuFrontEnd take; numBeams is set
  // to the laser's beam count.
  std::vector<double> RayCastScans(const lslam_laser& laser, const std::vector<Pose2>& sensorPoses, double maxRange,
                                   int* numBeams = nullptr) const {
    const double v = (laser.maximum_angle - laser.minimum_angle) / laser.angular_resolution;  // Karto.h:4152-4161
    const int n = static_cast<int>(v >= 0.0 ? std::floor(v + 0.5) : std::ceil(v - 0.5));
    if (numBeams) *numBeams = n;
    std::vector<double> xyh(sensorPoses.size() * 3), out(sensorPoses.size() * static_cast<size_t>(n > 0 ? n : 0));
    for (size_t i = 0; i < sensorPoses.size(); i++) {
      xyh[3 * i] = sensorPoses[i].x; xyh[3 * i + 1] = sensorPoses[i].y; xyh[3 * i + 2] = sensorPoses[i].heading;
    }
    Check(lslam_occgrid_ray_cast_scans(og_, &laser, static_cast<int>(sensorPoses.size()), xyh.data(), maxRange, out.data(), n));
    return out;
  }
  // calls, rays, cell-plane refreshes, samples tested
  std::vector<int64_t> Stats() const {
    std::vector<int64_t> s(4, 0);
    lslam_occgrid_ray_cast_stats(og_, s.data());
    return s;
  }
  lslam_occgrid* Grid() const { return og_; }

 private:
  void Check(int rc) const {
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  lslam_occgrid* og_;
};

// Batched many-scan mode over every GPU of the node (one process): scans sharded [r*B/W, (r+1)*B/W), shared grid
// replicated over xGMI, results in scan order
class GpuMatcherPool {
 public:
  GpuMatcherPool(int nDevices, const lslam_matcher_config& cfg, const lslam_laser& laser) {
    int rc = lslam_pool_create(nDevices, &cfg, &laser, &h_);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_pool_last_error(nullptr));
  }
  GpuMatcherPool(const std::vector<int>& devices, const lslam_matcher_config& cfg, const lslam_laser& laser) {
    int rc = lslam_pool_create_on(devices.data(), (int)devices.size(), &cfg, &laser, &h_);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_pool_last_error(nullptr));
  }
  ~GpuMatcherPool() { lslam_pool_destroy(h_); }
  GpuMatcherPool(const GpuMatcherPool&) = delete;
  GpuMatcherPool& operator=(const GpuMatcherPool&) = delete;
  int devices() const { return lslam_pool_devices(h_); }
  // ScanMatcher::AddScans once; the grid travels device-to-device
  void AddScans(const std::vector<RangeScan>& baseScans, int numBeams, const Pose2& center, bool rebuildEverywhere = false) {
    std::vector<double> r(baseScans.size() * (size_t)numBeams), p(baseScans.size() * 3);
    for (size_t i = 0; i < baseScans.size(); i++) {
      std::copy(baseScans[i].ranges, baseScans[i].ranges + numBeams, r.begin() + i * (size_t)numBeams);
      p[3 * i] = baseScans[i].sensor_pose.x; p[3 * i + 1] = baseScans[i].sensor_pose.y; p[3 * i + 2] = baseScans[i].sensor_pose.heading;
    }
    const double c[3] = {center.x, center.y, center.heading};
    int rc = lslam_pool_set_base_scans(h_, (int)baseScans.size(), r.data(), numBeams, p.data(), c, rebuildEverywhere ? 1 : 0);
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_pool_last_error(h_));
  }
  // the search part of MatchScan for n independent scans (ranges: n rows of numBeams doubles, poses: n*3)
  std::vector<lslam_match_result> MatchBatch(const double* ranges, int numBeams, const double* sensorPoses, int n,
                                             bool doPenalize = true, bool doRefineMatch = true) {
    std::vector<lslam_match_result> out((size_t)n);
    int rc = lslam_pool_match_batch(h_, n, ranges, numBeams, sensorPoses, doPenalize, doRefineMatch, out.data());
    if (rc != LSLAM_OK) throw MatcherError(rc, lslam_pool_last_error(h_));
    return out;
  }

 private:
  lslam_pool* h_ = nullptr;
};

// hectorslam::MapRepresentationInterface on the GPU: matchData + updateByScan
class MapRepGpu {
 public:
  // MapRepMultiMap(mapResolution, mapSizeX, mapSizeY, numDepth, startCoords)
  // (H/slam_main/MapRepMultiMap.h:57-93): offset = totalMapSize * startCoords
  MapRepGpu(lslam_context* ctx, float mapResolution, int mapSizeX, int mapSizeY, unsigned numDepth, float startX,
            float startY)
      : ctx_(ctx) {
    float offX = (mapResolution * static_cast<float>(mapSizeX)) * startX;
    float offY = (mapResolution * static_cast<float>(mapSizeY)) * startY;
    int rc = lslam_map_create(ctx, mapSizeX, mapSizeY, mapResolution, offX, offY, (int)numDepth, &h_);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx));
  }
  ~MapRepGpu() { lslam_map_destroy(h_); }
  MapRepGpu(const MapRepGpu&) = delete;
  MapRepGpu& operator=(const MapRepGpu&) = delete;

  void reset() { lslam_map_reset(h_); }
  float getScaleToMap() const { return lslam_map_scale_to_map(h_, 0); }
  int getMapLevels() const { return lslam_map_levels(h_); }
  void setUpdateFactorFree(float f) { lslam_map_set_update_factor_free(h_, f); }
  void setUpdateFactorOccupied(float f) { lslam_map_set_update_factor_occupied(h_, f); }
  // updateByScan(dataContainer, robotPoseWorld): points = DataContainer entries (x,y pairs, map-cell
  // units), origo = DataContainer::getOrigo()
  void updateByScan(const float* pointsXY, int n, const float origo[2], const float robotPoseWorld[3]) {
    int rc = lslam_map_update_by_scan(h_, pointsXY, n, origo, robotPoseWorld);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  // Eigen::Vector3f matchData(beginEstimateWorld, dataContainer, covMatrix)
  // (the container is cached for the levels above 0 of the next updateByScan, like MapRepMultiMap.h:161)
  void matchData(const float beginEstimateWorld[3], const float* pointsXY, int n, const float origo[2], float outPose[3],
                 float outCov[9]) {
    int rc = lslam_map_match_data(h_, pointsXY, n, origo, beginEstimateWorld, outPose, outCov);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  // Many matchData calls against the map as it is, in one launch: entry e = (container entryContainer[e], start pose
  // beginEstimatesWorld[e]); entryContainer == nullptr: entry i uses container i.  pointsXY: the containers back to back,
  // nPoints[nContainers].  A pure query: NO container is cached (the next updateByScan still feeds the levels above 0
  // from the last matchData's).  outCovs may be nullptr.
  void matchDataBatch(int nEntries, const float* beginEstimatesWorld, int nContainers, const float* pointsXY,
                      const int32_t* nPoints, const int32_t* entryContainer, float* outPoses, float* outCovs) {
    int rc = lslam_map_match_batch(h_, nEntries, nContainers, pointsXY, nPoints, entryContainer, beginEstimatesWorld, outPoses,
                                   outCovs);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  // float getLikelihoodForState(state, dataPoints) (H/map/OccGridMapUtil.h:342-347) for many states at once: entry e =
  // (container entryContainer[e], WORLD pose statesWorld[e]) on `level` of the map as it is.  outResiduals
  // (getResidualForState, :357-374) may be nullptr.  Containers as for matchDataBatch.  A pure query.
  void getLikelihoodForStates(int nEntries, const float* statesWorld, int nContainers, const float* pointsXY,
                              const int32_t* nPoints, const int32_t* entryContainer, int level, float* outLikelihoods,
                              float* outResiduals = nullptr) {
    int rc = lslam_map_score_batch(h_, nEntries, nContainers, pointsXY, nPoints, entryContainer, statesWorld, level, outResiduals,
                                   outLikelihoods);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  // Eigen::Matrix3f getCovarianceForPose(mapPose, dataPoints) (:249-306) and getCovMatrixWorldCoords (:314-339) for many
  // poses at once (WORLD poses; the sigma points are taken on the level's raster): outLikelihoods[nEntries][7],
  // outCovMap / outCovWorld [nEntries][9] row-major, either may be nullptr.
  void getCovarianceForPoses(int nEntries, const float* posesWorld, int nContainers, const float* pointsXY, const int32_t* nPoints,
                             const int32_t* entryContainer, int level, float* outLikelihoods, float* outCovMap,
                             float* outCovWorld) {
    int rc = lslam_map_pose_covariance_batch(h_, nEntries, nContainers, pointsXY, nPoints, entryContainer, posesWorld, level,
                                             outLikelihoods, outCovMap, outCovWorld);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  // getLikelihoodForState over the lattice centreWorld + (i - nx/2, j - ny/2, k - nt/2) * steps of one container:
  // outVolume[nt][ny][nx]; returns the best state's linear index (-1: every likelihood is NaN), its likelihood in
  // *outBestLikelihood when given.
  int scoreLattice(const float* pointsXY, int n, const float centreWorld[3], const int32_t counts[3], const float steps[3],
                   int level, float* outVolume, float* outBestLikelihood = nullptr) {
    int32_t best = -1;
    int rc = lslam_map_score_lattice(h_, pointsXY, n, centreWorld, counts, steps, level, outVolume, &best, outBestLikelihood);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
    return best;
  }
  // getGridMap(level) contents: log-odds plane / the int8 data of nav_msgs::OccupancyGrid
  void readLogOdds(int level, float* out) { lslam_map_read_logodds(h_, level, out); }
  void readOccupancy(int level, int8_t* out) { lslam_map_read_occupancy_i8(h_, level, out); }
  // the inverse of readLogOdds: a saved plane back in, or -- writeLogOddsDev with another map's plane in HBM -- a snapshot
  void writeLogOdds(int level, const float* plane) {
    if (lslam_map_write_logodds(h_, level, plane) != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  void writeLogOddsDev(int level, const float* planeDev) {
    if (lslam_map_write_logodds_dev(h_, level, planeDev) != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_map* handle() { return h_; }

 private:
  lslam_context* ctx_;
  lslam_map* h_ = nullptr;
};

// hectorslam::HectorSlamProcessor (H/slam_main/HectorSlamProcessor.h:57-117) streamed on the GPU: the match, the update
// decision and the update of every level stay on the device (lslam_hector_*), one host synchronisation per call.  Owns its
// MapRepGpu like the reference's processor owns its MapRepMultiMap (:61).  Use it where a stretch of scans is at hand
// (a recorded log, a queue that has run full); HectorMapRepGpu (integration/hector_map_rep_gpu.hpp) is for the reference's
// own processor driving the device one call at a time.
class LidarUndistortionGpu;
class HectorSlamProcessorGpu {
 public:
  // HectorSlamProcessor(mapResolution, mapSizeX, mapSizeY, startCoords, multi_res_size) (:57-68) + the device context
  HectorSlamProcessorGpu(lslam_context* ctx, float mapResolution, int mapSizeX, int mapSizeY, float startX, float startY,
                         int multi_res_size)
      : ctx_(ctx), map_(ctx, mapResolution, mapSizeX, mapSizeY, (unsigned)multi_res_size, startX, startY) {
    check(lslam_hector_create(map_.handle(), &h_));
  }
  ~HectorSlamProcessorGpu() { lslam_hector_destroy(h_); }
  HectorSlamProcessorGpu(const HectorSlamProcessorGpu&) = delete;
  HectorSlamProcessorGpu& operator=(const HectorSlamProcessorGpu&) = delete;

  // void update(const DataContainer& dataContainer, const Eigen::Vector3f& poseHintWorld, bool map_without_matching = false)
  // (:81) for any container with getSize() / getVecEntry(i) / getOrigo() and any pose indexable by [0..2]
  template <typename Container, typename Pose>
  void update(const Container& dataContainer, const Pose& poseHintWorld, bool map_without_matching = false) {
    const int n = dataContainer.getSize();
    pts_.resize((size_t)2 * (n > 0 ? n : 1));
    for (int i = 0; i < n; ++i) {
      pts_[(size_t)2 * i] = dataContainer.getVecEntry(i)[0];
      pts_[(size_t)2 * i + 1] = dataContainer.getVecEntry(i)[1];
    }
    const float origo[2] = {dataContainer.getOrigo()[0], dataContainer.getOrigo()[1]};
    const float hint[3] = {poseHintWorld[0], poseHintWorld[1], poseHintWorld[2]};
    const int32_t count = n;
    updateMany(1, pts_.data(), &count, origo, hint, &map_without_matching, nullptr);
  }
  // update() for nScans containers back to back (nPoints[nScans], origos nScans x 2 or nullptr = 0); poseHints == nullptr:
  // every scan starts from the previous result (hector_slam.cc:200-204); records may be nullptr
  void updateMany(int nScans, const float* pointsXY, const int32_t* nPoints, const float* origosXY, const float* poseHints,
                  const bool* mapWithoutMatching, lslam_hector_record* records) {
    flags_.assign((size_t)(nScans > 0 ? nScans : 0), 0);
    for (int k = 0; k < nScans && mapWithoutMatching; ++k) flags_[(size_t)k] = mapWithoutMatching[k] ? 1 : 0;
    check(lslam_hector_process_many_points(h_, nScans, pointsXY, nPoints, origosXY, poseHints,
                                           mapWithoutMatching ? flags_.data() : nullptr, records));
  }
  // update() for nScans RAW LaserScans that lesson5 de-skews first (LidarUndistortionGpu::CorrectLaserScans' inputs): one
  // batched de-skew launch for the call, then cloud -> DataContainer (rosPointCloudToDataContainer with `scan`'s filters and
  // laser transform), match, mark and apply per scan -- still one host synchronisation.  lesson5's cloud has z ~ 1: the z
  // window of `scan` must contain 1 or every container is empty.
  void updateManyDeskewed(const lslam_hector_scan& scan, int nScans, int nReadings, const float* ranges, int rangesStride,
                          const lslam_deskew_params* params, const int32_t* imuFirst, const double* imuTime,
                          const double* imuRotX, const double* imuRotY, const double* imuRotZ, const float* poseHints,
                          const bool* mapWithoutMatching, lslam_hector_record* records) {
    flags_.assign((size_t)(nScans > 0 ? nScans : 0), 0);
    for (int k = 0; k < nScans && mapWithoutMatching; ++k) flags_[(size_t)k] = mapWithoutMatching[k] ? 1 : 0;
    check(lslam_hector_process_many_deskewed(h_, &scan, nScans, nReadings, ranges, rangesStride, params, imuFirst, imuTime,
                                             imuRotX, imuRotY, imuRotZ, poseHints,
                                             mapWithoutMatching ? flags_.data() : nullptr, records));
  }
  // update() for nScans clouds that are de-skewed already (LidarUndistortionGpu::CorrectLaserScans' / ScanCallbacks' layout:
  // xyz nScans x nPoints x 3, valid nScans x nPoints or nullptr = every point).  take[nScans] (nullptr = all): a scan with
  // take false never reaches update() -- nothing of the processor changes, its record is zero with n_points = -1
  void updateManyClouds(const lslam_hector_scan& scan, int nScans, int nPoints, const float* xyz, const uint8_t* valid,
                        const bool* take, const float* poseHints, const bool* mapWithoutMatching, lslam_hector_record* records) {
    setFlags(nScans, mapWithoutMatching);
    take_.assign((size_t)(nScans > 0 ? nScans : 0), 0);
    for (int k = 0; k < nScans && take; ++k) take_[(size_t)k] = take[k] ? 1 : 0;
    check(lslam_hector_process_many_clouds(h_, &scan, nScans, nPoints, xyz, valid, take ? take_.data() : nullptr, poseHints,
                                           mapWithoutMatching ? flags_.data() : nullptr, records));
  }
  // the same on clouds in HBM (CorrectLaserScansDev's output); scan k is taken iff takeDev[k * takeStride] > 0 (nullptr = all):
  // &recordsDev[0].status of lslam_msync_record with takeStride = sizeof(lslam_msync_record) / 4 serves as it stands
  void updateManyCloudsDev(const lslam_hector_scan& scan, int nScans, int nPoints, const float* xyzDev, const uint8_t* validDev,
                           const int32_t* takeDev, int takeStride, const float* poseHints, const bool* mapWithoutMatching,
                           lslam_hector_record* records) {
    setFlags(nScans, mapWithoutMatching);
    check(lslam_hector_process_many_clouds_dev(h_, &scan, nScans, nPoints, xyzDev, validDev, takeDev, takeStride, poseHints,
                                               mapWithoutMatching ? flags_.data() : nullptr, records));
  }
  // lesson5's node in front of update(): nMsgs ScanCallbacks of `node` (its ImuCallback(s) / OdomCallback(s) before), the
  // scan each one corrects straight into update() on the device; a scan the node refuses never reaches it.  records[k] and
  // syncRecords[k] (either may be nullptr) belong to callback k.  One host synchronisation.  (Defined below the node.)
  inline void updateManySynced(LidarUndistortionGpu& node, const lslam_hector_scan& scan, const lslam_msync_laser& laser, int nMsgs,
                               int nReadings, const float* ranges, int rangesStride, const double* stamps,
                               const float* timeIncrements, const int64_t* imuSeen, const int64_t* odomSeen, const float* poseHints,
                               const bool* mapWithoutMatching, lslam_hector_record* records, lslam_msync_record* syncRecords);
  void reset() { check(lslam_hector_reset(h_)); }  // :111-117
  // getLastScanMatchPose / getLastScanMatchCovariance (:120-122)
  void getLastScanMatchPose(float out[3]) { check(lslam_hector_state(h_, out, nullptr, nullptr)); }
  void getLastScanMatchCovariance(float out[9]) { check(lslam_hector_state(h_, nullptr, out, nullptr)); }
  void getLastMapUpdatePose(float out[3]) { check(lslam_hector_state(h_, nullptr, nullptr, out)); }
  float getScaleToMap() const { return map_.getScaleToMap(); }
  int getMapLevels() const { return map_.getMapLevels(); }
  void setUpdateFactorFree(float f) { map_.setUpdateFactorFree(f); }
  void setUpdateFactorOccupied(float f) { map_.setUpdateFactorOccupied(f); }
  void setMapUpdateMinDistDiff(float d) { minDist_ = d; check(lslam_hector_set_update_thresholds(h_, minDist_, minAngle_)); }
  void setMapUpdateMinAngleDiff(float a) { minAngle_ = a; check(lslam_hector_set_update_thresholds(h_, minDist_, minAngle_)); }
  MapRepGpu& mapRep() { return map_; }
  lslam_hector* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  void setFlags(int nScans, const bool* mapWithoutMatching) {
    flags_.assign((size_t)(nScans > 0 ? nScans : 0), 0);
    for (int k = 0; k < nScans && mapWithoutMatching; ++k) flags_[(size_t)k] = mapWithoutMatching[k] ? 1 : 0;
  }
  lslam_context* ctx_;
  MapRepGpu map_;
  lslam_hector* h_ = nullptr;
  float minDist_ = 0.4f, minAngle_ = 0.13f;
  std::vector<float> pts_;
  std::vector<uint8_t> flags_, take_;
};

// R HectorSlamProcessorGpu advanced together (lslam_hector_fleet_*): one robot's scan k+1 needs its scan k, but robots need
// nothing of one another, so a STEP -- one scan of every member -- costs the launches of one processor's scan.  Either owns
// its processors (all of one construction) or borrows the caller's (any mix of map sizes, resolutions and depths; they must
// outlive the fleet).  Between calls every member is a HectorSlamProcessorGpu like any other.
class HectorSlamFleetGpu {
 public:
  // nMembers x HectorSlamProcessor(mapResolution, mapSizeX, mapSizeY, startCoords, multi_res_size)
  HectorSlamFleetGpu(lslam_context* ctx, int nMembers, float mapResolution, int mapSizeX, int mapSizeY, float startX, float startY,
                     int multi_res_size)
      : ctx_(ctx) {
    for (int r = 0; r < nMembers; ++r) {
      owned_.emplace_back(new HectorSlamProcessorGpu(ctx, mapResolution, mapSizeX, mapSizeY, startX, startY, multi_res_size));
      members_.push_back(owned_.back().get());
    }
    create();
  }
  // the caller's processors, borrowed
  HectorSlamFleetGpu(lslam_context* ctx, HectorSlamProcessorGpu* const* members, int nMembers)
      : ctx_(ctx), members_(members, members + (nMembers > 0 ? nMembers : 0)) {
    create();
  }
  ~HectorSlamFleetGpu() { lslam_hector_fleet_destroy(h_); }  // (before owned_: the fleet goes first)
  HectorSlamFleetGpu(const HectorSlamFleetGpu&) = delete;
  HectorSlamFleetGpu& operator=(const HectorSlamFleetGpu&) = delete;

  int size() const { return (int)members_.size(); }
  HectorSlamProcessorGpu& member(int r) { return *members_[(size_t)r]; }

  // HectorSlamProcessor::update (:81) for one step: dataContainers[r] / poseHintsWorld[r] are member r's, in the reference's
  // shapes (getSize() / getVecEntry(i) / getOrigo(); a pose indexable by [0..2]).  active: size() flags or nullptr = all; a
  // member that is not active is not touched (its container is not read).
  template <typename Container, typename Pose>
  void update(const Container* dataContainers, const Pose* poseHintsWorld, bool map_without_matching = false,
              const bool* active = nullptr, lslam_hector_record* records = nullptr) {
    const int R = size();
    pts_.clear();
    counts_.assign((size_t)R, 0);
    origos_.assign((size_t)2 * R, 0.f);
    hints_.assign((size_t)3 * R, 0.f);
    for (int r = 0; r < R; ++r) {
      if (active && !active[r]) continue;
      const Container& c = dataContainers[r];
      const int n = c.getSize();
      counts_[(size_t)r] = n;
      for (int i = 0; i < n; ++i) {
        pts_.push_back(c.getVecEntry(i)[0]);
        pts_.push_back(c.getVecEntry(i)[1]);
      }
      origos_[(size_t)2 * r] = c.getOrigo()[0];
      origos_[(size_t)2 * r + 1] = c.getOrigo()[1];
      for (int q = 0; q < 3; ++q) hints_[(size_t)3 * r + q] = poseHintsWorld[r][q];
    }
    flags_.assign((size_t)R, map_without_matching ? 1 : 0);
    active_.assign((size_t)R, 1);
    for (int r = 0; r < R && active; ++r) active_[(size_t)r] = active[r] ? 1 : 0;
    if (pts_.empty()) pts_.resize(2);
    updateMany(1, pts_.data(), counts_.data(), origos_.data(), hints_.data(), flags_.data(), active ? active_.data() : nullptr,
               records);
  }
  // nSteps steps of containers back to back, every per-scan array indexed step * size() + member as
  // lslam_hector_fleet_process_many_points takes them; poseHints == nullptr: every member chains from its own last pose
  void updateMany(int nSteps, const float* pointsXY, const int32_t* nPoints, const float* origosXY, const float* poseHints,
                  const uint8_t* mapWithoutMatching, const uint8_t* active, lslam_hector_record* records) {
    check(lslam_hector_fleet_process_many_points(h_, nSteps, pointsXY, nPoints, origosXY, poseHints, mapWithoutMatching, active,
                                                 records));
  }
  // the same for LaserScans of one geometry: ranges row step * size() + member
  void updateManyScans(const lslam_hector_scan& scan, int nSteps, int nReadings, const float* ranges, int rangesStride,
                       const float* poseHints, const uint8_t* mapWithoutMatching, const uint8_t* active,
                       lslam_hector_record* records) {
    check(lslam_hector_fleet_process_many(h_, &scan, nSteps, nReadings, ranges, rangesStride, poseHints, mapWithoutMatching,
                                          active, records));
  }
  // The gated forms (HectorSlamProcessorGpu::updateManyClouds / updateManyCloudsDev / updateManySynced for size() robots per
  // launch); every per-scan array indexed step * size() + member.  An entry is taken iff active (nullptr = all) and its take
  // flag (nullptr = all) say so; one that is not changes nothing of its member, its record is zero with n_points = -1.
  void updateManyClouds(const lslam_hector_scan& scan, int nSteps, int nPoints, const float* xyz, const uint8_t* valid,
                        const uint8_t* take, const float* poseHints, const uint8_t* mapWithoutMatching, const uint8_t* active,
                        lslam_hector_record* records) {
    check(lslam_hector_fleet_process_many_clouds(h_, &scan, nSteps, nPoints, xyz, valid, take, poseHints, mapWithoutMatching, active,
                                                 records));
  }
  // clouds in HBM: xyzDev / validDev / takeDev are host arrays of size() device pointers, one block per member (member m's
  // row of step k is k rows into its block); validDev, takeDev or single entries of them may be nullptr
  void updateManyCloudsDev(const lslam_hector_scan& scan, int nSteps, int nPoints, const float* const* xyzDev,
                           const uint8_t* const* validDev, const int32_t* const* takeDev, int takeStride, const float* poseHints,
                           const uint8_t* mapWithoutMatching, const uint8_t* active, lslam_hector_record* records) {
    check(lslam_hector_fleet_process_many_clouds_dev(h_, &scan, nSteps, nPoints, xyzDev, validDev, takeDev, takeStride, poseHints,
                                                     mapWithoutMatching, active, records));
  }
  // raw messages in: nodes[size()] are the members' lesson5 nodes (their ImuCallback(s) / OdomCallback(s) before); member m's
  // ScanCallbacks of the call are its steps with active != 0.  The synchronisation and the de-skew of all members run in 5
  // launches per call.  records / syncRecords (either may be nullptr): [nSteps * size()].  (Defined below the node.)
  inline void updateManySynced(LidarUndistortionGpu* const* nodes, const lslam_hector_scan& scan, const lslam_msync_laser& laser,
                               int nSteps, int nReadings, const float* ranges, int rangesStride, const double* stamps,
                               const float* timeIncrements, const int64_t* imuSeen, const int64_t* odomSeen, const float* poseHints,
                               const uint8_t* mapWithoutMatching, const uint8_t* active, lslam_hector_record* records,
                               lslam_msync_record* syncRecords);
  // {synced calls, launches of the fleet's synchronisation kernels, buffer growths, host waits}
  void syncStats(int64_t out[4]) const { lslam_hector_fleet_sync_stats(h_, out); }
  // {steps, member-scans, map updates, calls, host waits, launches of the fleet's kernels}
  void stats(int64_t out[6]) const { lslam_hector_fleet_stats(h_, out); }
  lslam_hector_fleet* handle() { return h_; }

 private:
  void create() {
    std::vector<lslam_hector*> hs;
    for (HectorSlamProcessorGpu* p : members_) hs.push_back(p ? p->handle() : nullptr);
    check(lslam_hector_fleet_create(hs.data(), (int)hs.size(), &h_));
  }
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  std::vector<std::unique_ptr<HectorSlamProcessorGpu>> owned_;
  std::vector<HectorSlamProcessorGpu*> members_;
  lslam_hector_fleet* h_ = nullptr;
  std::vector<float> pts_, origos_, hints_;
  std::vector<int32_t> counts_;
  std::vector<uint8_t> flags_, active_;
};

// R robots LOCALISING on one finished map (lslam_hector_loc_*): per robot and scan, HectorSlamProcessor::update (:81-108) with
// the gate never firing -- matchData from the hint or the robot's own last pose, lastScanMatchPose / lastScanMatchCov set, no
// updateByScan.  The map is borrowed and only read: it must outlive the localiser, and may be changed through its own methods
// (or a HectorSlamProcessorGpu on it) between calls.  A call costs 2 launches per chunk of steps (1 in the container form)
// whatever size() is, and one host wait.
class HectorLocalizerGpu {
 public:
  HectorLocalizerGpu(lslam_context* ctx, MapRepGpu& map, int nTrackers) : ctx_(ctx), n_(nTrackers) {
    check(lslam_hector_loc_create(map.handle(), nTrackers, &h_));
  }
  ~HectorLocalizerGpu() { lslam_hector_loc_destroy(h_); }
  HectorLocalizerGpu(const HectorLocalizerGpu&) = delete;
  HectorLocalizerGpu& operator=(const HectorLocalizerGpu&) = delete;

  int size() const { return n_; }
  // lastScanMatchPose of trackers first .. first + count - 1 (x, y, heading each); after construction: zero
  void setPoses(int first, int count, const float* posesXYH) { check(lslam_hector_loc_set_poses(h_, first, count, posesXYH)); }
  void getLastScanMatchPose(int tracker, float out[3]) { check(lslam_hector_loc_state(h_, tracker, out, nullptr)); }
  void getLastScanMatchCovariance(int tracker, float out[9]) { check(lslam_hector_loc_state(h_, tracker, nullptr, out)); }
  void setMaxStepsPerLaunch(int steps) { check(lslam_hector_loc_set_option(h_, LSLAM_HECTOR_LOC_OPT_MAX_STEPS_PER_LAUNCH, steps)); }

  // one step in the reference's shapes: dataContainers[r] is tracker r's (getSize() / getVecEntry(i)); poseHintsWorld[r]
  // indexable by [0..2], or nullptr: every tracker starts from its own last pose.  active: size() flags or nullptr = all.
  template <typename Container, typename Pose>
  void update(const Container* dataContainers, const Pose* poseHintsWorld = nullptr, const bool* active = nullptr,
              lslam_hector_record* records = nullptr) {
    pts_.clear();
    counts_.assign((size_t)n_, 0);
    hints_.assign((size_t)3 * n_, 0.f);
    active_.assign((size_t)n_, 1);
    for (int r = 0; r < n_; ++r) {
      if (active && !active[r]) {
        active_[(size_t)r] = 0;
        continue;
      }
      const Container& c = dataContainers[r];
      counts_[(size_t)r] = c.getSize();
      for (int i = 0; i < c.getSize(); ++i) {
        pts_.push_back(c.getVecEntry(i)[0]);
        pts_.push_back(c.getVecEntry(i)[1]);
      }
      for (int q = 0; q < 3 && poseHintsWorld; ++q) hints_[(size_t)3 * r + q] = poseHintsWorld[r][q];
    }
    if (pts_.empty()) pts_.resize(2);
    updateMany(1, pts_.data(), counts_.data(), poseHintsWorld ? hints_.data() : nullptr, active ? active_.data() : nullptr, records);
  }
  // nSteps steps; every per-entry array indexed step * size() + tracker, as the lslam_hector_loc_process_many* calls take them
  void updateMany(int nSteps, const float* pointsXY, const int32_t* nPoints, const float* poseHints, const uint8_t* active,
                  lslam_hector_record* records) {
    check(lslam_hector_loc_process_many_points(h_, nSteps, pointsXY, nPoints, poseHints, active, records));
  }
  void updateManyScans(const lslam_hector_scan& scan, int nSteps, int nReadings, const float* ranges, int rangesStride,
                       const float* poseHints, const uint8_t* active, lslam_hector_record* records) {
    check(lslam_hector_loc_process_many(h_, &scan, nSteps, nReadings, ranges, rangesStride, poseHints, active, records));
  }
  void updateManyClouds(const lslam_hector_scan& scan, int nSteps, int nPoints, const float* xyz, const uint8_t* valid,
                        const uint8_t* take, const float* poseHints, const uint8_t* active, lslam_hector_record* records) {
    check(lslam_hector_loc_process_many_clouds(h_, &scan, nSteps, nPoints, xyz, valid, take, poseHints, active, records));
  }
  // clouds in HBM, entry-major; takeDev: int32 words takeStride apart (lslam_msync_record::status at 22), or nullptr
  void updateManyCloudsDev(const lslam_hector_scan& scan, int nSteps, int nPoints, const float* xyzDev, const uint8_t* validDev,
                           const int32_t* takeDev, int takeStride, const float* poseHints, const uint8_t* active,
                           lslam_hector_record* records) {
    check(lslam_hector_loc_process_many_clouds_dev(h_, &scan, nSteps, nPoints, xyzDev, validDev, takeDev, takeStride, poseHints,
                                                   active, records));
  }
  // {steps, tracker-scans matched, calls, host waits, kernel launches, launches of the tracking kernel}
  void stats(int64_t out[6]) const { lslam_hector_loc_stats(h_, out); }
  lslam_hector_loc* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  int n_;
  lslam_hector_loc* h_ = nullptr;
  std::vector<float> pts_, hints_;
  std::vector<int32_t> counts_;
  std::vector<uint8_t> active_;
};

// LidarUndistortion::CorrectLaserScan (lesson5/src/lidar_undistortion.cc:339-447) for many scans per launch.  The caller
// of CorrectLaserScans* keeps what the node's callbacks and Prune* steps produce -- per scan the header, the odometry increment
// and the integrated IMU samples -- and hands a stretch of scans over at once; every scan's cloud is bit for bit what
// lslam_deskew_scan returns for it.  ImuCallback / OdomCallback / ScanCallback(s) are the whole node (:82-125): they keep
// those too, on the device.
class LidarUndistortionGpu {
 public:
  // useImu / useOdom: the node's parameters (:27-28); they matter to the callbacks below only
  explicit LidarUndistortionGpu(lslam_context* ctx, bool useImu = true, bool useOdom = true)
      : ctx_(ctx), use_imu_(useImu), use_odom_(useOdom) {
    check(lslam_deskew_create(ctx, &h_));
  }
  ~LidarUndistortionGpu() {
    lslam_msync_destroy(sync_);
    lslam_deskew_destroy(h_);
  }
  LidarUndistortionGpu(const LidarUndistortionGpu&) = delete;
  LidarUndistortionGpu& operator=(const LidarUndistortionGpu&) = delete;

  // nScans scans of nReadings beams (row k at ranges + k * rangesStride), one geometry; scan k owns the IMU samples
  // [imuFirst[k], imuFirst[k + 1]).  outXYZ: nScans x nReadings x 3 (corrected_pointcloud_'s x, y, z; zeros where the
  // reference skips a beam), outValid: nScans x nReadings.
  void CorrectLaserScans(int nScans, int nReadings, const float* ranges, int rangesStride, const lslam_deskew_params* params,
                         const int32_t* imuFirst, const double* imuTime, const double* imuRotX, const double* imuRotY,
                         const double* imuRotZ, float* outXYZ, uint8_t* outValid) {
    check(lslam_deskew_batch(h_, nScans, nReadings, ranges, rangesStride, params, imuFirst, imuTime, imuRotX, imuRotY, imuRotZ,
                             outXYZ, outValid));
  }
  // the same with ranges, outXYZ and outValid in HBM: asynchronous on lslam_stream(ctx), no host wait
  void CorrectLaserScansDev(int nScans, int nReadings, const float* rangesDev, int rangesStride,
                            const lslam_deskew_params* params, const int32_t* imuFirst, const double* imuTime,
                            const double* imuRotX, const double* imuRotY, const double* imuRotZ, float* outXYZDev,
                            uint8_t* outValidDev) {
    check(lslam_deskew_batch_dev(h_, nScans, nReadings, rangesDev, rangesStride, params, imuFirst, imuTime, imuRotX, imuRotY,
                                 imuRotZ, outXYZDev, outValidDev));
  }
  // {scans de-skewed, kernel launches, buffer growths, host waits}
  void stats(int64_t out[4]) const { lslam_deskew_stats(h_, out); }
  lslam_deskew* handle() { return h_; }

  // ---- the node's own shape: raw messages in, de-skewed clouds out (lslam_msync; the queues, their fronts, the sticky
  // start / end odometry messages and the one queued scan live on the device) ----
  struct Clouds {
    std::vector<float> xyz;                   // nMsgs x nReadings x 3; row k: the scan callback k corrected (message k - 1)
    std::vector<uint8_t> valid;               // nMsgs x nReadings
    std::vector<lslam_msync_record> records;  // nMsgs: status (LSLAM_MSYNC_*), times, odometry increment, fronts
  };
  // sensor_msgs/Imu: header.stamp and angular_velocity (:82-86)
  void ImuCallback(double stamp, double wx, double wy, double wz) {
    const double w[3] = {wx, wy, wz};
    check(lslam_msync_push_imu(sync(), 1, &stamp, w));
  }
  void ImuCallbacks(int n, const double* stamps, const double* gyroXYZ) { check(lslam_msync_push_imu(sync(), n, stamps, gyroXYZ)); }
  // nav_msgs/Odometry: header.stamp, pose.pose.position and orientation (x, y, z, w) (:89-93)
  void OdomCallback(double stamp, const double posXYZ[3], const double quatXYZW[4]) {
    check(lslam_msync_push_odom(sync(), 1, &stamp, posXYZ, quatXYZW));
  }
  void OdomCallbacks(int n, const double* stamps, const double* posXYZ, const double* quatXYZW) {
    check(lslam_msync_push_odom(sync(), n, stamps, posXYZ, quatXYZW));
  }
  // One sensor_msgs/LaserScan (:96-125) with every message pushed so far in the queues.  Returns the record; outXYZ
  // (nReadings x 3) and outValid (nReadings) hold the cloud of the PREVIOUS scan, zeros while the node queues or waits.
  lslam_msync_record ScanCallback(const lslam_msync_laser& laser, int nReadings, const float* ranges, double stamp,
                                  float timeIncrement, float* outXYZ, uint8_t* outValid) {
    lslam_msync_record rec;
    check(lslam_msync_scans(sync(), h_, &laser, 1, nReadings, ranges, nReadings, &stamp, &timeIncrement, nullptr, nullptr, outXYZ,
                            outValid, &rec));
    return rec;
  }
  // A stretch of LaserScans in one call.  imuSeen[k] / odomSeen[k]: how many IMU / odometry messages had arrived when scan
  // callback k ran (NULL: all of them).
  Clouds ScanCallbacks(const lslam_msync_laser& laser, int nMsgs, int nReadings, const float* ranges, int rangesStride,
                       const double* stamps, const float* timeIncrements, const int64_t* imuSeen = nullptr,
                       const int64_t* odomSeen = nullptr) {
    Clouds out;
    out.xyz.resize((size_t)nMsgs * nReadings * 3);
    out.valid.resize((size_t)nMsgs * nReadings);
    out.records.resize((size_t)nMsgs);
    check(lslam_msync_scans(sync(), h_, &laser, nMsgs, nReadings, ranges, rangesStride, stamps, timeIncrements, imuSeen, odomSeen,
                            out.xyz.data(), out.valid.data(), out.records.data()));
    return out;
  }
  void Reset() { check(lslam_msync_reset(sync())); }
  // {scan callbacks, scans corrected, scans refused, launches of the synchronisation's kernels, buffer growths, host waits}
  void syncStats(int64_t out[6]) { check(lslam_msync_stats(sync(), out)); }
  lslam_msync* syncHandle() { return sync(); }  // for HectorSlamProcessorGpu::updateManySynced

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_msync* sync() {  // made by the first callback: CorrectLaserScans* alone needs none
    if (!sync_) check(lslam_msync_create(ctx_, use_imu_, use_odom_, &sync_));
    return sync_;
  }
  lslam_context* ctx_;
  bool use_imu_ = true, use_odom_ = true;
  lslam_deskew* h_ = nullptr;
  lslam_msync* sync_ = nullptr;
};

inline void HectorSlamProcessorGpu::updateManySynced(LidarUndistortionGpu& node, const lslam_hector_scan& scan,
                                                     const lslam_msync_laser& laser, int nMsgs, int nReadings, const float* ranges,
                                                     int rangesStride, const double* stamps, const float* timeIncrements,
                                                     const int64_t* imuSeen, const int64_t* odomSeen, const float* poseHints,
                                                     const bool* mapWithoutMatching, lslam_hector_record* records,
                                                     lslam_msync_record* syncRecords) {
  setFlags(nMsgs, mapWithoutMatching);
  check(lslam_hector_process_many_synced(h_, node.syncHandle(), &scan, &laser, nMsgs, nReadings, ranges, rangesStride, stamps,
                                         timeIncrements, imuSeen, odomSeen, poseHints,
                                         mapWithoutMatching ? flags_.data() : nullptr, records, syncRecords));
}

inline void HectorSlamFleetGpu::updateManySynced(LidarUndistortionGpu* const* nodes, const lslam_hector_scan& scan,
                                                 const lslam_msync_laser& laser, int nSteps, int nReadings, const float* ranges,
                                                 int rangesStride, const double* stamps, const float* timeIncrements,
                                                 const int64_t* imuSeen, const int64_t* odomSeen, const float* poseHints,
                                                 const uint8_t* mapWithoutMatching, const uint8_t* active,
                                                 lslam_hector_record* records, lslam_msync_record* syncRecords) {
  std::vector<lslam_msync*> syncs;
  for (int r = 0; r < size() && nodes; ++r) syncs.push_back(nodes[r] ? nodes[r]->syncHandle() : nullptr);
  check(lslam_hector_fleet_process_many_synced(h_, nodes ? syncs.data() : nullptr, &scan, &laser, nSteps, nReadings, ranges,
                                               rangesStride, stamps, timeIncrements, imuSeen, odomSeen, poseHints,
                                               mapWithoutMatching, active, records, syncRecords));
}

// lesson1's LaserScan (lesson1/src/feature_detection.cc): ScanCallback's corner extraction, for one scan or many per
// launch.  cornerRanges is what the node publishes as corner_scan.ranges (its first n entries): the range of every
// picked beam, +0.0f elsewhere.  Among equal curvatures the higher compacted index ranks first (lslam_gpu.h).
class LaserScanFeaturesGpu {
 public:
  explicit LaserScanFeaturesGpu(lslam_context* ctx, float edgeThreshold = 1.0f) : ctx_(ctx) {
    check(lslam_features_create(ctx, &h_));
    const int rc = lslam_features_set_threshold(h_, edgeThreshold);
    if (rc != LSLAM_OK) {
      lslam_features_destroy(h_);
      check(rc);
    }
  }
  ~LaserScanFeaturesGpu() { lslam_features_destroy(h_); }
  LaserScanFeaturesGpu(const LaserScanFeaturesGpu&) = delete;
  LaserScanFeaturesGpu& operator=(const LaserScanFeaturesGpu&) = delete;

  // one scan of n beams; outIndex (120 original beam indices, -1 = unused slot) and outRecord may be NULL
  void ScanCallback(const float* ranges, int n, float* cornerRanges, int32_t* outIndex = nullptr,
                    lslam_feature_record* outRecord = nullptr) {
    ScanCallbacks(1, n, ranges, n, cornerRanges, outIndex, outRecord);
  }
  // nScans scans of nReadings beams (row k at ranges + k * rangesStride).  cornerRanges: nScans x nReadings, outIndex:
  // nScans x 120, outRecords: nScans; outIndex, outRecords and outCurvature (nScans x nReadings) may be NULL.
  void ScanCallbacks(int nScans, int nReadings, const float* ranges, int rangesStride, float* cornerRanges,
                     int32_t* outIndex = nullptr, lslam_feature_record* outRecords = nullptr, float* outCurvature = nullptr) {
    if (nScans > 0 && !outIndex) {
      index_.resize((size_t)nScans * LSLAM_FEATURE_SECTORS * LSLAM_FEATURE_PICKS);
      outIndex = index_.data();
    }
    if (nScans > 0 && !outRecords) {
      records_.resize((size_t)nScans);
      outRecords = records_.data();
    }
    check(lslam_features_batch(h_, nScans, nReadings, ranges, rangesStride, cornerRanges, outIndex, outRecords, outCurvature));
  }
  // the same with ranges and every output in HBM (outIndexDev and outRecordsDev are required here): asynchronous on
  // lslam_stream(ctx), no host wait
  void ScanCallbacksDev(int nScans, int nReadings, const float* rangesDev, int rangesStride, float* cornerRangesDev,
                        int32_t* outIndexDev, lslam_feature_record* outRecordsDev, float* outCurvatureDev = nullptr) {
    check(lslam_features_batch_dev(h_, nScans, nReadings, rangesDev, rangesStride, cornerRangesDev, outIndexDev, outRecordsDev,
                                   outCurvatureDev));
  }
  // {scans extracted, kernel launches, buffer growths, host waits}
  void stats(int64_t out[4]) const { lslam_features_stats(h_, out); }
  lslam_features* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  lslam_features* h_ = nullptr;
  std::vector<int32_t> index_;
  std::vector<lslam_feature_record> records_;
};

// lesson3's ScanMatchPLICP (lesson3/src/scan_match_plicp.cc) on the GPU: ScanCallback matches every scan against the one
// before it (ScanMatchWithPLICP :266-300, zero first guess); MatchPairs is the batch form.  Parity with the reference is
// unpinned (its arithmetic is the un-vendored csm); the results are defined by tools/plicp_cpu.py (see lslam_gpu.h).
class ScanMatchPLICPGpu {
 public:
  // the LaserScan header fields LaserScanToLDP reads; params NULL = the node's InitParams
  ScanMatchPLICPGpu(lslam_context* ctx, double angleMin, double angleIncrement, double rangeMin, double rangeMax,
                    const lslam_plicp_params* params = nullptr)
      : ctx_(ctx) {
    lslam_plicp_params p;
    if (params) p = *params; else lslam_plicp_params_defaults(&p);
    check(lslam_plicp_create(ctx, &p, &h_));
    const int rc = lslam_plicp_set_laser(h_, angleMin, angleIncrement, rangeMin, rangeMax);
    if (rc != LSLAM_OK) {
      lslam_plicp_destroy(h_);
      check(rc);
    }
  }
  ~ScanMatchPLICPGpu() { lslam_plicp_destroy(h_); }
  ScanMatchPLICPGpu(const ScanMatchPLICPGpu&) = delete;
  ScanMatchPLICPGpu& operator=(const ScanMatchPLICPGpu&) = delete;

  // One scan of n beams.  The first scan only becomes the previous one (false, *out zeroed: initialized_, :205-214);
  // afterwards *out is the pose of this scan in the previous scan's frame, and this scan becomes the previous one.  Every
  // scan must have the first one's beam count (std::invalid_argument otherwise).  Both scans of the pair go up with each call;
  // a log that is there as a whole is cheaper through MatchConsecutive.
  bool ScanCallback(const float* ranges, int n, lslam_plicp_record* out) {
    std::memset(out, 0, sizeof *out);
    if (n < 0 || !ranges) throw std::invalid_argument("ScanMatchPLICPGpu::ScanCallback: a scan is required");
    if (!initialized_) {
      prev_.assign(ranges, ranges + n);
      initialized_ = true;
      return false;
    }
    if ((int)prev_.size() != n) throw std::invalid_argument("ScanMatchPLICPGpu::ScanCallback: the beam count changed");
    two_.resize(2 * (size_t)n);
    std::memcpy(two_.data(), prev_.data(), (size_t)n * sizeof(float));
    std::memcpy(two_.data() + n, ranges, (size_t)n * sizeof(float));
    const int32_t ref = 0, sens = 1;
    check(lslam_plicp_match_batch(h_, 2, n, two_.data(), n, 1, &ref, &sens, nullptr, out));
    prev_.assign(ranges, ranges + n);
    return true;
  }
  // nPairs pairs over nScans scans (row k at ranges + k * rangesStride): pair b = scan pairSens[b] against scan pairRef[b];
  // firstGuess (nPairs x 3) may be NULL
  void MatchPairs(int nScans, int nReadings, const float* ranges, int rangesStride, int nPairs, const int32_t* pairRef,
                  const int32_t* pairSens, const double* firstGuess, lslam_plicp_record* out) {
    check(lslam_plicp_match_batch(h_, nScans, nReadings, ranges, rangesStride, nPairs, pairRef, pairSens, firstGuess, out));
  }
  // every scan against the one before it: out has nScans - 1 records
  void MatchConsecutive(int nScans, int nReadings, const float* ranges, int rangesStride, lslam_plicp_record* out) {
    if (nScans < 2) return;
    idx_.resize((size_t)nScans);
    for (int k = 0; k < nScans; k++) idx_[k] = k;
    MatchPairs(nScans, nReadings, ranges, rangesStride, nScans - 1, idx_.data(), idx_.data() + 1, nullptr, out);
  }
  // The same on clouds in the de-skew's layout (xyz: nClouds x nPoints x 3 float32, valid: nClouds x nPoints bytes or NULL):
  // a point takes part iff its valid byte is set and x, y are finite, its reading index is its position; the constructor's
  // laser is not read.  This is how a de-skewed scan (lesson5) is matched.
  void MatchClouds(int nClouds, int nPoints, const float* xyz, const uint8_t* valid, int nPairs, const int32_t* pairRef,
                   const int32_t* pairSens, const double* firstGuess, lslam_plicp_record* out) {
    check(lslam_plicp_match_clouds(h_, nClouds, nPoints, xyz, valid, nPairs, pairRef, pairSens, firstGuess, out));
  }
  // clouds, valid bytes, first guesses and records in HBM; asynchronous on lslam_stream(), no host wait
  void MatchCloudsDev(int nClouds, int nPoints, const float* xyzDev, const uint8_t* validDev, int nPairs, const int32_t* pairRef,
                      const int32_t* pairSens, const double* firstGuessDev, lslam_plicp_record* outDev) {
    check(lslam_plicp_match_clouds_dev(h_, nClouds, nPoints, xyzDev, validDev, nPairs, pairRef, pairSens, firstGuessDev, outDev));
  }
  // {pairs matched, kernel launches, buffer growths, host waits}
  void stats(int64_t out[4]) const { lslam_plicp_stats(h_, out); }
  lslam_plicp* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  lslam_plicp* h_ = nullptr;
  bool initialized_ = false;
  std::vector<float> prev_, two_;
  std::vector<int32_t> idx_;
};

// lesson3's keyframe odometry node (lesson3/src/plicp_odometry.cc) on the GPU for nTracks independent tracks.
class PlicpOdometryGpu {
 public:
  PlicpOdometryGpu(lslam_context* ctx, int nTracks, double angleMin, double angleIncrement, double rangeMin, double rangeMax,
                   const double baseToLaser[3] = nullptr, double kfDistLinear = 0.1,
                   double kfDistAngular = 5.0 * (3.14159265358979323846 / 180.0), int kfScanCount = 10,
                   const lslam_plicp_params* params = nullptr)
      : ctx_(ctx), tracks_(nTracks) {
    lslam_plicp_params p;
    if (params) p = *params; else lslam_plicp_params_defaults(&p);
    check(lslam_plicp_odom_create(ctx, &p, nTracks, kfDistLinear, kfDistAngular, kfScanCount, baseToLaser, &h_));
    const int rc = lslam_plicp_odom_set_laser(h_, angleMin, angleIncrement, rangeMin, rangeMax);
    if (rc != LSLAM_OK) {
      lslam_plicp_odom_destroy(h_);
      check(rc);
    }
  }
  ~PlicpOdometryGpu() { lslam_plicp_odom_destroy(h_); }
  PlicpOdometryGpu(const PlicpOdometryGpu&) = delete;
  PlicpOdometryGpu& operator=(const PlicpOdometryGpu&) = delete;

  // one scan of a one-track odometry (ScanCallback, :191-232)
  void ScanCallback(const float* ranges, int n, double stamp, lslam_plicp_odom_record* out) {
    ProcessMany(1, n, ranges, n, &stamp, nullptr, out);
  }
  // nSteps scans per track, every per-scan array indexed step * nTracks + track; active may be NULL (all 1)
  void ProcessMany(int nSteps, int nReadings, const float* ranges, int rangesStride, const double* stamps,
                   const uint8_t* active, lslam_plicp_odom_record* out) {
    check(lslam_plicp_odom_process_many(h_, nSteps, nReadings, ranges, rangesStride, stamps, active, out));
  }
  // The node on clouds (xyz: nSteps x nTracks x nPoints x 3 float32, valid: bytes per point or NULL), gated: an entry is taken
  // iff active (NULL: all) and take (bytes, NULL: all) say so; one that is not changes nothing of its track (record: zero with
  // iterations = -1).  Between Reset()s an odometry runs either ProcessMany or ProcessClouds[Dev], with one point count.
  void ProcessClouds(int nSteps, int nPoints, const float* xyz, const uint8_t* valid, const uint8_t* take, const double* stamps,
                     const uint8_t* active, lslam_plicp_odom_record* out) {
    check(lslam_plicp_odom_process_many_clouds(h_, nSteps, nPoints, xyz, valid, take, stamps, active, out));
  }
  // The same on clouds in HBM: nTracks device pointers each, one block per track; take words are int32, taken iff > 0,
  // takeStride words apart (22 on &records[0].status of lslam_msync_record).  stamps, active and out are host arrays.
  void ProcessCloudsDev(int nSteps, int nPoints, const float* const* xyzDev, const uint8_t* const* validDev,
                        const int32_t* const* takeDev, int takeStride, const double* stamps, const uint8_t* active,
                        lslam_plicp_odom_record* out) {
    check(lslam_plicp_odom_process_many_clouds_dev(h_, nSteps, nPoints, xyzDev, validDev, takeDev, takeStride, stamps, active, out));
  }
  void Reset() { check(lslam_plicp_odom_reset(h_)); }
  // out: nTracks states
  void State(lslam_plicp_odom_track* out) { check(lslam_plicp_odom_state(h_, out)); }
  int tracks() const { return tracks_; }
  // {scans processed, kernel launches, buffer growths, host waits}
  void stats(int64_t out[4]) const { lslam_plicp_odom_stats(h_, out); }
  lslam_plicp_odom* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  int tracks_;
  lslam_plicp_odom* h_ = nullptr;
};

// lesson2's ScanMatchICP (lesson2/src/scan_match_icp.cc) on the GPU: ScanCallback keeps the last scan and aligns its cloud
// (the source) to the current scan's (the target), as ScanMatchWithICP (:135-164) does with a default-configured
// pcl::IterativeClosestPoint; MatchPairs is the batch form.  Parity with the reference is unpinned (its arithmetic is PCL's);
// the results are defined by tools/icp_cpu.py (see lslam_gpu.h).
class ScanMatchICPGpu {
 public:
  // the LaserScan header fields ConvertScan2PointCloud reads; params NULL = PCL's defaults
  ScanMatchICPGpu(lslam_context* ctx, double angleMin, double angleIncrement, double rangeMin, double rangeMax,
                  const lslam_icp_params* params = nullptr)
      : ctx_(ctx) {
    lslam_icp_params p;
    if (params) p = *params; else lslam_icp_params_defaults(&p);
    check(lslam_icp_create(ctx, &p, &h_));
    const int rc = lslam_icp_set_laser(h_, angleMin, angleIncrement, rangeMin, rangeMax);
    if (rc != LSLAM_OK) {
      lslam_icp_destroy(h_);
      check(rc);
    }
  }
  ~ScanMatchICPGpu() { lslam_icp_destroy(h_); }
  ScanMatchICPGpu(const ScanMatchICPGpu&) = delete;
  ScanMatchICPGpu& operator=(const ScanMatchICPGpu&) = delete;

  // One scan of n beams.  The first scan only becomes the last one (false, *out zeroed: is_first_scan_, :56-62); afterwards
  // *out is the transformation of the last scan's cloud onto this one's, and this scan becomes the last one.  The node prints
  // the transformation only where out->converged is set (:148-163).  Every scan must have the first one's beam count.
  bool ScanCallback(const float* ranges, int n, lslam_icp_record* out) {
    std::memset(out, 0, sizeof *out);
    if (n < 0 || !ranges) throw std::invalid_argument("ScanMatchICPGpu::ScanCallback: a scan is required");
    if (!initialized_) {
      last_.assign(ranges, ranges + n);
      initialized_ = true;
      return false;
    }
    if ((int)last_.size() != n) throw std::invalid_argument("ScanMatchICPGpu::ScanCallback: the beam count changed");
    ScanMatchWithICP(ranges, n, out);
    last_.assign(ranges, ranges + n);
    return true;
  }
  // last -> current (:135-164)
  void ScanMatchWithICP(const float* ranges, int n, lslam_icp_record* out) {
    two_.resize(2 * (size_t)n);
    std::memcpy(two_.data(), last_.data(), (size_t)n * sizeof(float));
    std::memcpy(two_.data() + n, ranges, (size_t)n * sizeof(float));
    const int32_t source = 0, target = 1;
    check(lslam_icp_match_batch(h_, 2, n, two_.data(), n, 1, &source, &target, nullptr, out));
  }
  // nPairs pairs over nScans scans (row k at ranges + k * rangesStride): pair b aligns scan pairSource[b] to scan
  // pairTarget[b]; firstGuess (nPairs x 3: x, y, yaw) may be NULL
  void MatchPairs(int nScans, int nReadings, const float* ranges, int rangesStride, int nPairs, const int32_t* pairSource,
                  const int32_t* pairTarget, const double* firstGuess, lslam_icp_record* out) {
    check(lslam_icp_match_batch(h_, nScans, nReadings, ranges, rangesStride, nPairs, pairSource, pairTarget, firstGuess, out));
  }
  // every scan's cloud onto the next one's: out has nScans - 1 records
  void MatchConsecutive(int nScans, int nReadings, const float* ranges, int rangesStride, lslam_icp_record* out) {
    if (nScans < 2) return;
    idx_.resize((size_t)nScans);
    for (int k = 0; k < nScans; k++) idx_[k] = k;
    MatchPairs(nScans, nReadings, ranges, rangesStride, nScans - 1, idx_.data(), idx_.data() + 1, nullptr, out);
  }
  // {pairs matched, kernel launches, buffer growths, host waits}
  void stats(int64_t out[4]) const { lslam_icp_stats(h_, out); }
  lslam_icp* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  lslam_icp* h_ = nullptr;
  bool initialized_ = false;
  std::vector<float> last_, two_;
  std::vector<int32_t> idx_;
};

// lesson2's ScanToPointCloud2Converter (lesson2/src/scan_to_pointclod2_converter.cc) on the GPU: ScanCallback (:44-92) turns a
// scan into n points (x, y, z) of float32, an invalid reading into the node's invalid_point_ (NaN, NaN, NaN).
class ScanToPointCloud2ConverterGpu {
 public:
  ScanToPointCloud2ConverterGpu(lslam_context* ctx, double angleMin, double angleIncrement, double rangeMin, double rangeMax)
      : ctx_(ctx) {
    lslam_icp_params p;
    lslam_icp_params_defaults(&p);
    p.invalid_as_nan = 1;
    check(lslam_icp_create(ctx, &p, &h_));
    const int rc = lslam_icp_set_laser(h_, angleMin, angleIncrement, rangeMin, rangeMax);
    if (rc != LSLAM_OK) {
      lslam_icp_destroy(h_);
      check(rc);
    }
  }
  ~ScanToPointCloud2ConverterGpu() { lslam_icp_destroy(h_); }
  ScanToPointCloud2ConverterGpu(const ScanToPointCloud2ConverterGpu&) = delete;
  ScanToPointCloud2ConverterGpu& operator=(const ScanToPointCloud2ConverterGpu&) = delete;

  // one scan: xyz = n x 3 floats, valid = n bytes
  void ScanCallback(const float* ranges, int n, float* xyz, uint8_t* valid) { ConvertMany(1, n, ranges, n, xyz, valid); }
  // nScans scans in one launch (row k at ranges + k * rangesStride)
  void ConvertMany(int nScans, int nReadings, const float* ranges, int rangesStride, float* xyz, uint8_t* valid) {
    check(lslam_icp_convert_batch(h_, nScans, nReadings, ranges, rangesStride, xyz, valid));
  }
  lslam_icp* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  lslam_context* ctx_;
  lslam_icp* h_ = nullptr;
};

// gmapping::ScanMatcherMap (lesson4/include/lesson4/gmapping/grid/map.h) on the GPU, read side, plus the node's
// ComputeMap (gmapping.cc:171-242).  cell() reads from a host copy of the counters, refreshed after every change.
struct IntPoint2 {  // gmapping::IntPoint
  int x = 0, y = 0;
};
struct Point2 {  // gmapping::Point
  double x = 0, y = 0;
};
struct GpuPointAccumulator {  // gmapping::PointAccumulator (map.h:17-35)
  struct { float x = 0, y = 0; } acc;
  int n = 0, visits = 0;
  // visits ? n / visits : -1 (map.h:27)
  operator double() const { return visits ? (double)n * 1 / (double)visits : -1; }
};

class GpuScanMatcherMap {
 public:
  // ScanMatcherMap(center, xmin, ymin, xmax, ymax, delta) with center = the box's middle (gmapping.cc:130-135)
  GpuScanMatcherMap(lslam_context* ctx, double xmin, double ymin, double xmax, double ymax, double delta) : ctx_(ctx) {
    int rc = lslam_gmap_create(ctx, xmin, ymin, xmax, ymax, delta, &h_);
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx));
    lslam_gmap_info(h_, &g_);
  }
  ~GpuScanMatcherMap() { lslam_gmap_destroy(h_); }
  GpuScanMatcherMap(const GpuScanMatcherMap&) = delete;
  GpuScanMatcherMap& operator=(const GpuScanMatcherMap&) = delete;

  // GMapping::CreateCache + InitParams' maxRange / maxUrange
  void setLaser(int n_beams, float angle_min, float angle_increment, double max_range = 30 - 0.01,
                double max_use_range = 25.0) {
    check(lslam_gmap_set_laser(h_, n_beams, angle_min, angle_increment, max_range, max_use_range));
  }
  // GMapping::ComputeMap on a fresh map: the laser at (0, 0, 0)
  void ComputeMap(const float* ranges) {
    check(lslam_gmap_reset(h_));
    check(lslam_gmap_integrate(h_, 1, ranges, nullptr));
    stale_ = true;
  }
  // many scans at poses (x, y, theta) into this map
  void registerScans(int n_scans, const float* ranges, const double* poses) {
    check(lslam_gmap_integrate(h_, n_scans, ranges, poses));
    stale_ = true;
  }
  // PublishMap's data: width() x height() int8
  void publish(double occ_thresh, int8_t* out) { check(lslam_gmap_read_ros_i8(h_, occ_thresh, out)); }

  int getMapSizeX() const { return g_.map_size_x; }
  int getMapSizeY() const { return g_.map_size_y; }
  double getDelta() const { return g_.delta; }
  int width() const { return g_.width; }
  int height() const { return g_.height; }
  // Map::world2map / map2world (map.h:171-182)
  IntPoint2 world2map(const Point2& p) const {
    return {(int)std::round((p.x - g_.center_x) / g_.delta) + g_.size_x2,
            (int)std::round((p.y - g_.center_y) / g_.delta) + g_.size_y2};
  }
  Point2 map2world(const IntPoint2& p) const {
    return {(p.x - g_.size_x2) * g_.delta + g_.center_x, (p.y - g_.size_y2) * g_.delta + g_.center_y};
  }
  bool isInside(const IntPoint2& p) const { return p.x >= 0 && p.y >= 0 && p.x < g_.map_size_x && p.y < g_.map_size_y; }
  // const Map::cell(IntPoint): the cell, or the unknown cell outside the storage
  GpuPointAccumulator cell(const IntPoint2& p) {
    GpuPointAccumulator c;
    if (!isInside(p)) return c;
    refresh();
    const size_t i = (size_t)p.y * g_.map_size_x + p.x, cells = visits_.size();
    c.acc.x = acc_[i];
    c.acc.y = acc_[cells + i];
    c.n = n_[i];
    c.visits = visits_[i];
    return c;
  }
  lslam_gmap* handle() { return h_; }

 private:
  void check(int rc) {
    if (rc != LSLAM_OK) throw std::runtime_error(lslam_last_error(ctx_));
  }
  void refresh() {
    if (!stale_) return;
    const size_t cells = (size_t)g_.map_size_x * g_.map_size_y;
    visits_.resize(cells);
    n_.resize(cells);
    acc_.resize(2 * cells);
    check(lslam_gmap_read_counters(h_, visits_.data(), n_.data(), acc_.data()));
    stale_ = false;
  }
  lslam_context* ctx_;
  lslam_gmap* h_ = nullptr;
  lslam_gmap_geometry g_{};
  bool stale_ = true;
  std::vector<int32_t> visits_, n_;
  std::vector<float> acc_;
};

}  // namespace lslam
