/* Stand-in for cuML's handle type, so that the reference's Stixels class compiles without cuML.
 * Clustering is not part of what oracle/_ref/ pins (see ref_stubs/cuml/cluster/dbscan.hpp). */
#ifndef REF_STUB_CUML_HPP_
#define REF_STUB_CUML_HPP_
namespace ML {
class cumlHandle {};
}  // namespace ML
#endif
