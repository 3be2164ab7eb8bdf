/* diffspectra_tiles.h - launch-form switches of the sampling library (libdiffspectra_hip.so) that are no part of the denoiser's
 * interface in diffspectra_hip.h: they change which kernels a launch site picks, never a result.  Plain C, as the other headers;
 * read on the Python side by diffspectra_amd/abi.py (abi.TILES) and bound by engine.load_library(). */
#ifndef DIFFSPECTRA_TILES_H
#define DIFFSPECTRA_TILES_H

#ifdef __cplusplus
extern "C" {
#endif

/* Row-tile form of the node-row kernels of a block (k_node_update, k_node_qkv).  rows = 64: one 512-thread workgroup per 64 rows - every
 * weight fragment streamed from L2 serves two 32-row tiles, q|k|v normalises a tile once; rows = 32: the 32-row k_node_update and the
 * column-split q|k|v; -1: follow the environment variable DIFFSPECTRA_NODE_TILE if set, else 64 once the launch has four 64-row tiles
 * per compute unit.  Returns the previous setting.  Process-global, like ds_set_two_stream.  Results are bit-identical in both forms.
 * (Build extension: the reference has no such switch.) */
int ds_set_node_tile(int rows);

#ifdef __cplusplus
}
#endif
#endif /* DIFFSPECTRA_TILES_H */
