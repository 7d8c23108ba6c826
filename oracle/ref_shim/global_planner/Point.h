// ref_shim/global_planner/Point.h — TEST INFRASTRUCTURE ONLY: the one name utils.h takes from the global_planner
// package (a template argument of a helper no tested path instantiates).
#ifndef REF_SHIM_GLOBAL_PLANNER_POINT_H
#define REF_SHIM_GLOBAL_PLANNER_POINT_H
#include <cstddef>
namespace KDTree {
template <std::size_t N> struct Point {
    double v[N];
    double operator[](std::size_t i) const { return v[i]; }
};
}  // namespace KDTree
#endif
