/* Stand-in for cuML's DBSCAN: does nothing.  The reference's Stixels::ClusterInstances calls it
 * once per instance class after the DP; the labels it would write are not read by the driver.
 * DBSCAN itself is pinned against the reference's Python clustering instead
 * (tests/golden/reference_python/). */
#ifndef REF_STUB_CUML_DBSCAN_HPP_
#define REF_STUB_CUML_DBSCAN_HPP_
#include "../cuml.hpp"
namespace ML {
template <typename... Args>
inline void dbscanFit(const cumlHandle&, Args&&...) {}
}  // namespace ML
#endif
