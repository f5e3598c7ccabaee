// What the device headers of rgb-d-slam_amd/csrc need of <hip/hip_runtime.h> to compile as plain host C++ (tests/host/map_kalman_algebra.cpp):
// the function qualifiers as nothing and the vector types as structs.  Put this directory in front of the include path.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline

struct double2 { double x, y; };
struct uint2 { unsigned x, y; };
struct int2 { int x, y; };
inline double2 make_double2(double x, double y) { return {x, y}; }
typedef struct ihipStream_t* hipStream_t;
using std::isfinite;
