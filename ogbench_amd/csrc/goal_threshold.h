// goal_threshold.h -- the exact squared-distance bound of a norm test (host only,
// plain C++: tests/test_goal_threshold_cpu.py compiles it without HIP).
#pragma once

#include <cmath>
#include <limits>

namespace ogbx {

// The largest double s with fl(sqrt(s)) <= tol, for a finite tol >= 0.  sqrt is
// correctly rounded and monotone, so for every double s
//   fl(sqrt(s)) <= tol  <=>  s <= goal_s2max(tol)
// and the success test np.linalg.norm(xy - goal) <= tol needs no square root
// (as kPointFarD2 for the point radius).  Starts at fl(tol * tol), at most a
// few ulps off, and walks with nextafter.
inline double goal_s2max(double tol) {
  const double inf = std::numeric_limits<double>::infinity();
  double s = tol * tol;
  while (s > 0.0 && std::sqrt(s) > tol) s = std::nextafter(s, 0.0);
  while (std::sqrt(std::nextafter(s, inf)) <= tol) s = std::nextafter(s, inf);
  return s;
}

}  // namespace ogbx
