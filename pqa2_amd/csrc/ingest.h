// Launchers of ingest.hip (decoder surfaces -> planes).  Kept out of kernels.h: that header is part of the source hash
// that ties profiles/kernel_counters.json to the scoring kernels (bench.py kernel_source_hash).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pqa {

// 16-bit samples with the value in the upper bits (P010 / P012 luma) -> LSB-aligned u16 plane.  Pitches in bytes.
hipError_t launch_ingest_shift16(hipStream_t stream, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                                 void* dst, int64_t dst_row_pitch, int64_t dst_frame_pitch, int w, int h, int shift,
                                 int n_frames);
// Interleaved U,V pairs (NV12: esize 1, shift 0; P010 / P012: esize 2, shift 16 - bit depth) -> U plane and V plane of
// w x h samples each (same pitches for both).
hipError_t launch_ingest_deinterleave(hipStream_t stream, int esize, const void* src_uv, int64_t src_row_pitch,
                                      int64_t src_frame_pitch, void* dst_u, void* dst_v, int64_t dst_row_pitch,
                                      int64_t dst_frame_pitch, int w, int h, int shift, int n_frames);

// unpack.hip: packed 4:2:2 capture formats (include/pqa_vmaf.h, PQA_SURFACE_UYVY / _YUYV / _V210) -> Y, U, V planes of
// w x h and ceil(w / 2) x h samples (u8; v210: LSB-aligned u16).  dst[1] or dst[2] null: luma only, no chroma is decoded.
// Pitches in bytes.  hipErrorInvalidValue, before any launch, on a source row pitch below the format's minimum (host_packed.h), a v210
// source that is not made of whole 32-bit words, or a destination that is not made of whole samples.
enum { UNPACK_UYVY = 3, UNPACK_YUYV = 4, UNPACK_V210 = 5 };   // the PQA_SURFACE_* values
hipError_t launch_unpack(hipStream_t stream, int format, const void* src, int64_t src_row_pitch, int64_t src_frame_pitch,
                         void* const dst[3], const int64_t dst_row_pitch[3], const int64_t dst_frame_pitch[3], int w, int h,
                         int n_frames);

}  // namespace pqa
