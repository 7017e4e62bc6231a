// svgf_rough_table.h — what a svgf_rough_table is, for the two sources that read one: svgf_scene_rough.hip (libsvgf_rough.so), which
// creates and destroys it, and svgf_scene_highlight.hip (libsvgf_highlight.so), which is handed one and reads device, n and dev.
// Private, as svgf_gloss_table.h is: include/svgf_rough.h keeps the type opaque, and neither library exports anything for the other.
#ifndef SVGF_ROUGH_TABLE_H_
#define SVGF_ROUGH_TABLE_H_

#include "../../include/svgf_rough.h"
#include "svgf_device_table.h"

struct svgf_rough_table {
    int device, n;
    float *dev;                 // n values on `device` (null with n == 0)
};

#endif
