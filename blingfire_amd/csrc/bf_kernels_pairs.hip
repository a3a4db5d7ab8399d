// bf_kernels_pairs.hip -- pairs of ragged id sequences -> fixed-shape model inputs with type ids: the row stage (bf_rowstage_body.h has the kernels)
// over PairsSource (bf_pairs.h has the cell logic and what a row is).  A lane takes its pair's geometry from the four offsets again in every kernel.
#include "bf_rowstage_body.h"

namespace bfa {

template void launch_rowstage_count<PairsSource>(const RowStageParams<PairsSource> &p, hipStream_t s);
template void launch_rowstage_map<PairsSource>(const RowStageParams<PairsSource> &p, hipStream_t s);
template void launch_rowstage_fill<PairsSource>(const RowStageParams<PairsSource> &p, hipStream_t s);
template void launch_rowstage_planes<PairsSource>(const RowPlanesParams<PairsSource> &p, hipStream_t s);

} // namespace bfa
