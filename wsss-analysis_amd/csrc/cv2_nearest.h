// cv2_nearest.h -- the source index of cv2.resize(..., interpolation=INTER_NEAREST), shared by cam_tail.hip (the nearest-neighbour
// confusion entry points) and render.hip (wsc_render_labels).  OpenCV: inv_scale = 1. / (dsize / ssize) in double on the host,
// then per output index  min(cvFloor(x * inv_scale), ssize - 1).  One product and one floor: nothing here can be contracted.
#pragma once

inline double cv2_nearest_inv(int src, int out) { return 1.0 / ((double)out / (double)src); }

__device__ __forceinline__ int cv2_nearest_index(int x, double inv, int src) { return min((int)floor((double)x * inv), src - 1); }
