// Depth Pro (include/ovm3d.h, "Depth Pro, metric depth"): geometry shared by depthpro.hip and its host-side checks.
#pragma once
#include <string>

#include "../../include/ovm3d.h"

namespace ovm {

struct DepthProGeom {
  int crop = 0, g = 0, S = 0;          // crop side, token grid of a crop (= the base map side), network canvas 4 * crop
  int ncrop[3] = {0, 0, 0};            // crops per side at ratio 1, 0.5, 0.25 (5, 3, 1)
  int stride[3] = {0, 0, 0};           // crop stride in pixels of its level
  int pad[3] = {0, 0, 0};              // cells cut from inner crop borders when merging
  int merged[3] = {0, 0, 0};           // merged map side (before the resize to out[])
  int out[3] = {0, 0, 0};              // target side: 4 g, 2 g, g
  int total = 0;                       // 35
};

// Host only, no device call: the supported geometry or OVM_ERR_UNSUPPORTED / OVM_ERR_INVALID with a message.
int depthpro_geometry(const OvmDepthProConfig& c, DepthProGeom* geo, std::string* err);

}  // namespace ovm
