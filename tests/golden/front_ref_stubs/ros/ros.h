// ros/ros.h for make_front_ref_golden.cpp ONLY (it comes first on that driver's include path; tests/shim_stubs/ros/ros.h,
// which always answers `false`, stays what the shim compile test uses).  ros::param::get serves the values the driver
// put into front_ref_params() before it constructed PoseFuser / ScanPointResampler: their constructors are the only way
// to set delTime, coeVel, coeOmega, space and spaceThre (include/ndt_slam/PoseFuser.h:19-23, ScanPointResampler.h:19-22).
#pragma once
#include <cstdio>
#include <iostream>   // the real ros/ros.h brings it in: src/PoseFuser.cpp uses std::cout without including it
#include <map>
#include <string>
inline std::map<std::string, double> &front_ref_params() {
  static std::map<std::string, double> table;
  return table;
}
namespace ros { namespace param {
template <typename T> bool get(const std::string &key, T &value) {
  std::map<std::string, double> &t = front_ref_params();
  std::map<std::string, double>::const_iterator it = t.find(key);
  if (it == t.end()) return false;
  value = static_cast<T>(it->second);
  return true;
}
} }
#define ROS_INFO(...) ((void)0)
#define ROS_INFO_STREAM(x) ((void)0)
#define ROS_ERROR(...) ((void)0)
#define ROS_FATAL(...) ((void)0)
