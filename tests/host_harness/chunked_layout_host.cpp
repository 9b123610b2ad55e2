// The __host__ __device__ layout functions of csrc/chunked_sweep.h behind a C interface, built with the host compiler
// alone (tests/test_chunked_layout_host.py).
#include "../../audio_tokens_amd/csrc/chunked_sweep.h"

extern "C" {

int chunked_layout_host_slot(int r, int q, int h) { return cs::chunk_slot(r, q, h); }

unsigned chunked_layout_host_centroid_of(unsigned code, int h) { return cs::centroid_of(code, h); }

int chunked_layout_host_acc_base_plus_offset(int ai, int e, int h) { return cs::acc_base(ai, h) + cs::reg_offset(e); }

long long chunked_layout_host_tile_floats(int d, int na) { return (long long)at_chunked_image_tile_floats(d, na); }

int chunked_layout_host_buf_floats(int na) { return cs::buf_floats(na); }
}
