// Device-side view of the GRBM graph held by a dvg_graph handle.
#pragma once
#include <stdint.h>

#include "gibbs_plan.h"

struct dvg_graph {
  int n, n_edges, n_colours, max_degree, n_adj;
  int device;
  // device arrays (owned)
  int32_t *edge_i, *edge_j;      // [n_edges]
  int32_t *order;                // [n] spins in colour-class order
  int32_t *class_ptr;            // [n_colours + 1]
  int32_t *adj_ptr;              // [n + 1]
  int32_t *adj_idx, *adj_eid;    // [2 n_edges]
  // The sampler's LDS image of the neighbour lists (gibbs.hip): every CSR row padded to whole batches of 4 entries.
  // (shape.n_batches over all rows, shape.max_batches in the longest)
  int32_t *adj_row;              // [n]  (first batch of the row << 8) | its batches
  int32_t *adj_src4;             // [4 n_batches]  CSR position of the entry, -1 for padding
  // The fast schedule's LANE-MAJOR image (gibbs.hip::gibbs_fast_kernel), for the graphs gibbs_graph_shape gives one
  // (shape.lane_has; null otherwise), with lpc / mb / nr / rows = shape.lane_*.  A class of c spins takes ceil(c / lpc)
  // passes; passes are grouped in STEPS of nr rows (a class's last step may hold an empty row), rows = nr * steps rows in
  // all.  Row k of lane l: its spin lane_spin[k lpc + l] (-1: none) and, at entry ((k mb + j) lpc + l) 4 + e, neighbour
  // 4 j + e of that spin: lane_eid = its edge (-1: none), lane_off = the byte offset of its state inside a chain's float16
  // state row (0 for none).
  int32_t *lane_spin;            // [rows][lpc]
  int32_t *lane_eid;             // [rows][mb][lpc][4]
  uint16_t *lane_off;            // [rows][mb][lpc][4]
  dvg::GibbsGraphShape shape;    // what the draw's plan reads (gibbs_plan.h): host side only
};
