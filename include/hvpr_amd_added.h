/*
 * hvpr_amd — prototypes added to the C-ABI within an ABI version without touching the census of include/hvpr_amd.h that
 * tests/test_capi_symbols.py pins.  Part of hvpr_amd.h: included from there (inside its extern "C" block, after its typedefs) and
 * documented there, entry by entry; do not include it on its own.  hvpr_amd/_lib.py derives the binding of these entries from this
 * file exactly as it derives the others from hvpr_amd.h (ADDED_SIGNATURES / ADDED_PARAMS), and tests/test_pointpillar_host.py checks
 * that each is exported.  At the next ABI version the entries move into hvpr_amd.h and this file goes back to empty.
 */
#ifndef HVPR_AMD_ADDED_H
#define HVPR_AMD_ADDED_H

/* a2 (plain): see hvpr_amd.h */
int hvpr_pillar_vfe_plain_fwd_f32(const float *voxels, const int32_t *num_points, const int32_t *coords, int M, int P,
                                  const int32_t *m_device, float vs_x, float vs_y, float vs_z, float off_x, float off_y,
                                  float off_z, const float *w, const float *b, int c_out, float *pillar_features,
                                  float *pillar_mask, hvpr_stream_t stream);

#endif /* HVPR_AMD_ADDED_H */
