// svgf_gloss_table.h — what a svgf_gloss_table is, for the two sources that read one: svgf_scene_gloss.hip (libsvgf_gloss.so), which
// creates and destroys it, and svgf_scene_virtual.hip (libsvgf_virtual.so), which is handed one and reads device, n and dev.  Private:
// include/svgf_gloss.h keeps the type opaque, and neither library exports anything for the other (svgf_device_table.h: the create,
// destroy and size this table shares with svgf_rough_table.h's).
#ifndef SVGF_GLOSS_TABLE_H_
#define SVGF_GLOSS_TABLE_H_

#include "../../include/svgf_gloss.h"
#include "svgf_device_table.h"

struct svgf_gloss_table {
    int device, n;
    SvgfSurface *dev;           // n records on `device` (null with n == 0)
};

#endif
