// bf_kernels_rows.hip -- ragged ids -> fixed-shape model inputs: the row stage (bf_rowstage_body.h has the kernels) over RowsSource (bf_rows.h has
// the cell logic and what a row is), and the grid size every row-stage launch takes.
#include "bf_rowstage_body.h"

namespace bfa {

unsigned rows_blocks(int64_t items)
{
    int64_t blocks = (items + 255) / 256;
    if (blocks > (int64_t)device_cus() * 8) blocks = (int64_t)device_cus() * 8;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

template void launch_rowstage_count<RowsSource>(const RowStageParams<RowsSource> &p, hipStream_t s);
template void launch_rowstage_map<RowsSource>(const RowStageParams<RowsSource> &p, hipStream_t s);
template void launch_rowstage_fill<RowsSource>(const RowStageParams<RowsSource> &p, hipStream_t s);

} // namespace bfa
