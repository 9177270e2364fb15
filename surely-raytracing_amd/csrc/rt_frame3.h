// rt_frame3.h — the two vector helpers the ray generators form a view frame with: f = unit(forward),
// r = unit(f x up), u = r x f (rt_host.h). One definition for the host generator (host/capi.cpp,
// librthost) and for the device generator's host side (rt_raygen.hip, librtmi355x), so that the
// frame the kernel receives as arguments holds the bits of the frame the host loop uses. Plain
// C++, host only; both libraries are built without contraction, and / and sqrt round correctly.
#pragma once
#include <cmath>

namespace rtframe {

inline bool unit3(const double* v, double* out) {
  const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  if (!(n > 0.0) || !std::isfinite(n)) return false;
  for (int k = 0; k < 3; ++k) out[k] = v[k] / n;
  return true;
}
inline void cross3(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

}  // namespace rtframe
