/* libcm3d_reader.so: what the box size stage (include/cm3d_hip.h, cm3d_box_size) needs of the host-side loader beyond
 * include/cm3d_reader.h and include/cm3d_reader_velocity.h -- the result writer with a size per box.  Plain C; conventions as in
 * cm3d_reader.h. */
#ifndef CM3D_READER_SIZE_H
#define CM3D_READER_SIZE_H

#include "cm3d_reader.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cm3d_write_results_json with a size per record: size double[n][3] = [w, l, h], row i beside records row i, written as
 * '"size": [w, l, h]' with Python's repr() of the three floats (Infinity / -Infinity / NaN as json.dumps spells them).  The writer
 * puts '], "size": [w, l, h], "rotation": [' behind the translation's numbers itself, in place of cls_mid[class] (which must still
 * be given).  vel: NULL -- cls_score[class] as cm3d_write_results_json takes it --, or double[n][2] with cls_score as
 * cm3d_write_results_json_vel takes it.  Everything else, the return value included, as cm3d_write_results_json. */
int64_t cm3d_write_results_json_sized(const double *records, const double *vel, const double *size, int64_t n, const char *tokens,
                                      int32_t n_tokens, const char *const *cls_mid, const char *const *cls_score,
                                      const char *const *cls_tail, int32_t n_classes, const char *prefix, char *out, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* CM3D_READER_SIZE_H */
