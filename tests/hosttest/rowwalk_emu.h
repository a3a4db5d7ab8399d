// rowwalk_emu.h -- TEST-ONLY: the host counterpart of blingfire_amd/csrc/bf_rowwalk.h for the emulators of the per-row kernels.  A group of G lanes
// is an array of G values; a row is walked in chunks of G cells in order, lane l at cell j0 + l, and a cross-lane read takes all lanes' old values
// before any lane writes its new one.  (The loop over rows and chunks is two `for` lines in each emulator and stays there: nothing shared would
// make it shorter.)
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <vector>
#include "../../blingfire_amd/csrc/bf_mlm.h"

namespace bfa {

// what a lane holds of its cell for the whole-word head; a lane past the end of the row holds {-1, 0, false}
struct EmuHeadCell { int32_t S, E; bool eligible; };

// mlm_chunk_head over the G lanes of one chunk: the end and the "joins" flag one lane up (lane 0: the carry), the head by an inclusive max-scan
// in log2 G steps that read l - d "all at once", the close with the carried head, and the last lane's values as the next carry.  h[l] = the head
inline void emu_chunk_head(const EmuHeadCell *cell, int G, int j0, MlmCarry &carry, int *h)
{
    std::vector<int> joins((size_t)G), next((size_t)G);
    for (int l = 0; l < G; ++l) joins[(size_t)l] = mlm_joins(cell[l].eligible, cell[l].S) ? 1 : 0;
    for (int l = 0; l < G; ++l) {                 // one lane up; lane 0 takes the carry
        const int32_t end_prev = l ? cell[l - 1].E : carry.end;
        const int joins_prev = l ? joins[(size_t)l - 1] : carry.joins;
        h[l] = mlm_head_seed(mlm_continues(joins_prev != 0, end_prev, joins[(size_t)l] != 0, cell[l].S), j0 + l);
    }
    for (int d = 1; d < G; d <<= 1) {             // the scan: every lane reads d lanes up, all at once
        for (int l = 0; l < G; ++l) next[(size_t)l] = mlm_head_step(h[l], h[l >= d ? l - d : l], l >= d);
        for (int l = 0; l < G; ++l) h[l] = next[(size_t)l];
    }
    for (int l = 0; l < G; ++l) h[l] = mlm_head_close(h[l], carry.head);
    carry = MlmCarry{cell[G - 1].E, joins[(size_t)G - 1], h[G - 1]};
}

} // namespace bfa
