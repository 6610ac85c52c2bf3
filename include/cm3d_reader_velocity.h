/* libcm3d_reader.so: what the box velocity stage (include/cm3d_hip.h, cm3d_box_velocity) needs of the host-side loader beyond
 * include/cm3d_reader.h -- the sample table's `next` and `timestamp` for the batch assembly, and the result writer with a velocity
 * per box.  Plain C; conventions as in cm3d_reader.h (return 0 / CM3D_RD_OK or a negative CM3D_RD_ERR_*). */
#ifndef CM3D_READER_VELOCITY_H
#define CM3D_READER_VELOCITY_H

#include "cm3d_reader.h"

#ifdef __cplusplus
extern "C" {
#endif

/* For n rows of sample.json (as cm3d_tables_job_tokens and cm3d_manifest_copy's sample_index name them): next_row[i] = the row of
 * the sample's `next`, -1 for the last sample of a scene; timestamp[i] = its `timestamp`, microseconds, as the integer the file
 * holds.  A row outside the table: CM3D_RD_ERR_ARG and nothing written. */
int cm3d_tables_sample_links(const cm3d_tables *t, const int32_t *rows, int32_t n, int32_t *next_row, int64_t *timestamp);

/* cm3d_write_results_json with a velocity per record: vel double[n][2], row i beside records row i, written as
 * '"velocity": [vx, vy]' with Python's repr() of the two floats (Infinity / -Infinity / NaN as json.dumps spells them).  The
 * writer puts '], "velocity": [vx, vy' behind the rotation's numbers itself; cls_score[class] then starts at the bracket that
 * closes the velocity ('], "detection_name": ...').  Everything else, the return value included, as cm3d_write_results_json. */
int64_t cm3d_write_results_json_vel(const double *records, const double *vel, int64_t n, const char *tokens, int32_t n_tokens,
                                    const char *const *cls_mid, const char *const *cls_score, const char *const *cls_tail,
                                    int32_t n_classes, const char *prefix, char *out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* CM3D_READER_VELOCITY_H */
