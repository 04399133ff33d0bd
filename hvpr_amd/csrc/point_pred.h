// The per-point keep decisions of the KITTI pre-processing, shared by preprocess.hip (hvpr_point_flags_f32, one frame) and
// collate.hip (hvpr_ragged_select_*, a whole batch), so that both take THE SAME fp32 operations in the same order and decide
// bit-equally:
//   mask_points_by_range    pcdet/utils/common_utils.py:59-62 (x and y only, both ends inclusive)
//   FOV                     KittiDataset.get_fov_flag, pcdet/datasets/kitti/kitti_dataset.py:100-116 over
//                           Calibration.lidar_to_rect / rect_to_img, pcdet/utils/calibration_kitti.py:65-84 (all float32)
//   near flag               DataProcessor.sample_points, pcdet/datasets/processor/data_processor.py:87-88
// Both including files are compiled with -ffp-contract=off: no product below may fuse with its sum.
#pragma once

// ((x*m0 + y*m1) + z*m2) + 1*m3 of column j of a row-major 4 x 3 matrix, left to right
__device__ __forceinline__ float hvpr_dot4(float x, float y, float z, const float *m, int j) {
    return ((x * m[j] + y * m[3 + j]) + z * m[6 + j]) + m[9 + j];
}

__device__ __forceinline__ bool hvpr_pred_range_xy(float x, float y, float x0, float y0, float x1, float y1) {
    return x >= x0 && x <= x1 && y >= y0 && y <= y1;
}

// the near flag of DataProcessor.sample_points, data_processor.py:87-88: ||xyz||_2 < near, the squares summed left to right
__device__ __forceinline__ bool hvpr_pred_near(float x, float y, float z, float near) {
    return __fsqrt_rn((x * x + y * y) + z * z) < near;
}

// a: (V2C^T R0^T), rect_j = sum_i hom_i * a[i*3 + j];  p: P2^T, img_j = sum_i rhom_i * p[i*3 + j]
__device__ __forceinline__ bool hvpr_pred_fov(float x, float y, float z, const float *a, const float *p, float img_h, float img_w) {
    const float rx = hvpr_dot4(x, y, z, a, 0), ry = hvpr_dot4(x, y, z, a, 1), rz = hvpr_dot4(x, y, z, a, 2);
    const float hx = hvpr_dot4(rx, ry, rz, p, 0), hy = hvpr_dot4(rx, ry, rz, p, 1), hz = hvpr_dot4(rx, ry, rz, p, 2);
    const float u = __fdiv_rn(hx, rz), v = __fdiv_rn(hy, rz);       // divided by the rect depth (calibration_kitti.py:82)
    const float depth = hz - p[11];                                  // P2.T[3,2]
    return u >= 0.f && u < img_w && v >= 0.f && v < img_h && depth >= 0.f;
}
