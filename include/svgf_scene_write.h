/* svgf_scene_write.h — row f26: the prototypes of the two product entry points (libsvgf_hip.so) that let renderer-side code write the
 * resident scene's triangles as drawn and refit its tree on request.  include/svgf.h states their contract, under row f26; they are
 * added after 0.9: probe the symbol.  include/svgf_deform.h (libsvgf_deform.so) is their first user. */
#ifndef SVGF_SCENE_WRITE_H_
#define SVGF_SCENE_WRITE_H_

#include "svgf.h"

#ifdef __cplusplus
extern "C" {
#endif

int svgf_scene_drawn_arrays(svgf_scene *scene, float **tris_dev, SvgfBvhNode **tri_boxes_dev);
int svgf_scene_refit(svgf_scene *scene, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVGF_SCENE_WRITE_H_ */
