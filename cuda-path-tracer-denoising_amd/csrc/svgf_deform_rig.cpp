// svgf_deform_rig.cpp — row f26: svgf_deform_check_rig_host, the rig's validation (include/svgf_deform.h lists every refusal).  Plain
// C++ with no HIP in it, so that tests/native/deform_rig_main.cpp can compile it on its own under the sanitizers; libsvgf_deform.so
// runs it in svgf_deform_create before any device work, which is what keeps a bone index inside the table on the device.
#include "../../include/svgf_deform.h"

#include <cmath>

extern "C" int svgf_deform_check_rig_host(int n_tris, const int *tri_index, int n_skinned, const unsigned short *bone, const float *weight, int n_bones)
{
    if (!tri_index || !bone || !weight || n_tris < 1 || n_skinned < 1 || n_skinned > n_tris) return SVGF_ERR_INVALID_ARG;
    if (n_bones < 1 || n_bones > SVGF_DEFORM_MAX_BONES) return SVGF_ERR_INVALID_ARG;
    int before = -1;
    for (int s = 0; s < n_skinned; s++) {
        const int i = tri_index[s];
        if (i <= before || i >= n_tris) return SVGF_ERR_INVALID_ARG;       // strictly increasing from >= 0
        before = i;
    }
    for (long long k = 0; k < 12LL * n_skinned; k++) {
        if ((int)bone[k] >= n_bones) return SVGF_ERR_INVALID_ARG;
        if (!std::isfinite(weight[k]) || weight[k] < 0.0f) return SVGF_ERR_INVALID_ARG;
    }
    return SVGF_OK;
}
