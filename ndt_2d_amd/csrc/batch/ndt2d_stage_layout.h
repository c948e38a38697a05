// Where the pieces of one chunk's upload lie in the stage of the batched searches on the installed
// grid (scans/ndt2d_scans.hip match_chunk): [dth | dlin | beams | jobs | order | cos / sin rows],
// offsets and sizes in doubles.  The start poses of one scan (starts/) travel as 3-double records
// without an order table.  The beams are read with 16-byte loads, so they start on an even
// double; the order table holds 32-bit entries, two to a double, and the unused half of an odd
// last entry is the double in front of the rows (the host zeroes it: nothing undefined travels).
// Plain C++: host code and a stand-alone check include it without the HIP headers.
#ifndef NDT2D_STAGE_LAYOUT_H_
#define NDT2D_STAGE_LAYOUT_H_

#include <stddef.h>

namespace ndt2d
{

constexpr size_t kJobDoubles = 4;     // a job's record (JobRec, ndt2d_batch_search.h)
constexpr size_t kStartDoubles = 3;   // a start's (StartRec)

struct StageLayout
{
  size_t dth, dlin, beams, jobs, order, trig;   // the first double of each piece
  size_t total;
};

// n_beams: of all the scans the chunk sends; record_doubles: kJobDoubles or kStartDoubles;
// order_entries: n_slots, or 0 for no order table; trig_doubles: distinct headings x 2 x n_th.
inline StageLayout stage_layout(size_t n_th, size_t n_lin, size_t n_beams, size_t n_slots, size_t record_doubles,
                                size_t order_entries, size_t trig_doubles)
{
  StageLayout l;
  l.dth = 0;
  l.dlin = n_th;
  l.beams = (n_th + n_lin + 1) & ~size_t(1);
  l.jobs = l.beams + 2 * n_beams;
  l.order = l.jobs + n_slots * record_doubles;
  l.trig = l.order + (order_entries + 1) / 2;
  l.total = l.trig + trig_doubles;
  return l;
}

}  // namespace ndt2d

#endif  // NDT2D_STAGE_LAYOUT_H_
