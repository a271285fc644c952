// kbest_cluster_sample_partial.hip -- the second instantiation of kbest_cluster_sample.hip: the small clusters of a frame whose open
// clusters are drawn by kbest_frontier_sample.hip (kbest_hybrid_frontier_sample_assoc_batch_f64).  A translation unit of its own:
// the plain kernel's code object does not change.  gfx950, fp64, plain HIP C++.  DESIGN.md section 18.
#define KB_CLUSTER_SAMPLE_PARTIAL 1
#include "kbest_cluster_sample.hip"
