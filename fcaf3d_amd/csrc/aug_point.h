// The train pipeline's transform of ONE point, in the reference's order: GlobalAlignment (transforms_3d.py:409-490), RandomFlip3D
// (:59-170), GlobalRotScaleTrans (:493-645).  Shared by k_augment_voxelize (csrc/coords.hip, one launch per scene) and
// k_batch_augment_voxelize (csrc_post/batch.hip, one launch per batch), whose coords are bit-equal for the same rows.
//
// a (21 floats used): [0..8] alignment R (row-major; p' = R p + t), [9..11] t, [12] has_align, [13] flip x, [14] flip y,
// [15] cos(angle), [16] sin(angle), [17] scale, [18..20] translation.  Every step rounds to fp32 as the reference's tensor ops do:
// separate multiply / add, contraction switched off in the body whatever the including file has set.  Values in, values out: a form
// that takes the output pointers and stores through them reschedules the callers' address arithmetic (profiles/r7_notes.md).
#pragma once
#ifdef __HIP__                 // the host emulators (tools/*_host_emu.cpp) compile this text as plain C++ with the qualifiers defined away
#include <hip/hip_runtime.h>
#endif

struct AugP { float x, y, z; };

__device__ static inline AugP aug_point(float x, float y, float z, const float* a) {
#pragma clang fp contract(off)
  if (a[12] != 0.f) {                                   // GlobalAlignment: points.rotate(R^T) then translate
    const float nx = (x * a[0] + y * a[1]) + z * a[2];
    const float ny = (x * a[3] + y * a[4]) + z * a[5];
    const float nz = (x * a[6] + y * a[7]) + z * a[8];
    x = nx + a[9]; y = ny + a[10]; z = nz + a[11];
  }
  if (a[13] != 0.f) x = -x;                             // RandomFlip3D 'horizontal'
  if (a[14] != 0.f) y = -y;                             // ... 'vertical'
  {                                                     // GlobalRotScaleTrans: p @ rot_T, rot_T = [[c, s, 0], [-s, c, 0], [0, 0, 1]]
    const float c = a[15], sn = a[16];
    const float nx = x * c - y * sn;
    const float ny = x * sn + y * c;
    x = nx * a[17] + a[18];
    y = ny * a[17] + a[19];
    z = z * a[17] + a[20];
  }
  return AugP{x, y, z};
}
