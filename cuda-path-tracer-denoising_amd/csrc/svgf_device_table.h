// svgf_device_table.h — the one create / destroy / size behind svgf_gloss_table_* and svgf_rough_table_*: a table is
// { int device, n; Record *dev; }, n validated host records uploaded once to `device`.  Private, header-only and of internal
// linkage: neither library exports anything for the other.  Include behind svgf_kernels.h (SvgfDeviceGuard, the HIP runtime).
#ifndef SVGF_DEVICE_TABLE_H_
#define SVGF_DEVICE_TABLE_H_

#include "../../include/svgf.h"

#include <new>

// record_ok(const Record &) -> bool: the refusal of one record
template <class Table, class Record, class Ok>
static inline int svgf_device_table_create(int device, const Record *host, int n, Table **out, Ok record_ok)
{
    if (!out) return SVGF_ERR_INVALID_ARG;
    *out = nullptr;
    if (n < 0 || n > SVGF_SCENE_MAX_POSED || (n > 0 && !host) || device < 0) return SVGF_ERR_INVALID_ARG;
    for (int i = 0; i < n; i++)
        if (!record_ok(host[i])) return SVGF_ERR_INVALID_ARG;
    SvgfDeviceGuard dev_guard(device);
    if (!dev_guard.ok) {
        (void)hipGetLastError();        // a device that does not exist must not fail the next launch's check
        return SVGF_ERR_NO_DEVICE;
    }
    Table *t = new (std::nothrow) Table{ device, n, nullptr };
    if (!t) return SVGF_ERR_OOM;
    if (n > 0) {
        if (hipMalloc(reinterpret_cast<void **>(&t->dev), (size_t)n * sizeof(Record)) != hipSuccess) {
            (void)hipGetLastError();
            delete t;
            return SVGF_ERR_OOM;
        }
        if (hipMemcpy(t->dev, host, (size_t)n * sizeof(Record), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(t->dev);
            delete t;
            return SVGF_ERR_HIP;
        }
    }
    *out = t;
    return SVGF_OK;
}

template <class Table>
static inline void svgf_device_table_destroy(Table *t)
{
    if (!t) return;
    if (t->dev) {
        SvgfDeviceGuard dev_guard(t->device);
        (void)hipFree(t->dev);
    }
    delete t;
}

template <class Table>
static inline int svgf_device_table_size(const Table *t) { return t ? t->n : SVGF_ERR_INVALID_ARG; }

#endif
