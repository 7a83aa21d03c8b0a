// pack_image.h -- what npa_create derives from a configuration and a checkpoint WITHOUT a device: the polygon's vertices and
// the host image of the weight pack (layout: pan_common.h, WP_*).  Pure host arithmetic; pack_image.hip contains no kernel and
// calls nothing of the HIP runtime, so it also builds into a stand-alone host program (tests/tools/host/pack_image_check.cpp).
#pragma once
#include "../../include/neupan_amd.h"
#include "pan_common.h"

#include <vector>

// Vertices of {x : G x <= h} for the geometric distance keys, from P.E / P.G / P.h of a P that is otherwise zero-filled or set
// from the configuration: pvx / pvy / pdx / pdy / pil, geo_rect, and rc* / rh* (the box itself for an axis-aligned rectangle,
// the bounding box grown by 10 um for any other polygon).  Returns geo_valid: the rows are consecutive counter-clockwise edges.
bool npa_polygon_geometry(DevParams& P);

// The WP_TOTAL floats of the pack as they are uploaded: header of the key table (WP_TABH), +inf margins, and -- with weights --
// every weight layout.  w == nullptr (a planner without obstacle stage): header and margins only.
void npa_build_pack_image(const DevParams& P, bool geo_valid, const npa_dune_weights* w, std::vector<float>& image);
