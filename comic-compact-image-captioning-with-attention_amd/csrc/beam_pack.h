// Geometry of the packed output projection (beam_pack_wo_kernel, beam_logits.hip): shared by the beam step's streaming
// vocabulary projection and by the caption-scoring projection (score_logits.hip), so that there is ONE packed layout.
#pragma once

#ifndef BL_VT
#define BL_VT 7
#endif
// 16-column tiles per workgroup: 7 -> 112-column chunks, 229 workgroups at V = 25 599 (8 -> 200 of the 256 CUs)
constexpr int kVT = BL_VT;
constexpr int kChunkCols = 16 * kVT;    // vocabulary columns per workgroup
constexpr int kQuarterBytes = 4 * kVT * 2 * 1024;     // four k-steps of kVT tiles x {hi, lo} x 1 KB
