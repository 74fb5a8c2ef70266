// mat_storage.cpp -- storage-only stand-in for the four OpenCV library symbols that the reference's
// cv::Mat-allocating matching stages reach (SmoothConstraint, SetBoundary_smooth, MedianFilter, Rematch,
// LowestLevelInitialMatch):
//
//     cv::Mat::create(int, const int*, int)      allocate rows x cols elements and a reference counter
//     cv::Mat::operator=(const cv::Scalar&)      fill every element with a constant
//     cv::Mat::deallocate()                      free what create() allocated
//     cv::fastFree(void*)                        free() (the destructor names it for step.p; never taken for 2-D)
//
// THE RULE: storage management may be stood in for; anything that computes pixel values may not.  This file
// therefore does malloc, fill and free and nothing else -- no copy, convert, filter, resize or arithmetic on
// images.  Every other OpenCV symbol stays unresolved (the probe links with --unresolved-symbols=ignore-all),
// so a stage that needs more than storage cannot run instead of running on a fake.
//
// Written from the member layout the vendored OpenCV 2.4.5 headers declare for cv::Mat (flags, dims, rows,
// cols, data, refcount, datastart / dataend / datalimit, allocator, size, step), included where they lie;
// the header-inline parts of cv::Mat (constructors, release(), operator=(const Mat&), ptr<>()) stay the
// reference's own.  2-D matrices only; the fill handles CV_8U with 1-3 channels and CV_16S with 1 channel,
// the only types those stages allocate.  Anything else aborts with a message.
#define __declspec(x)
#define _Longlong long long
#include "SharedInclude.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static void unsupported(const char *what, int a, int b) {
    fprintf(stderr, "mat_storage: %s not stood in for (%d, %d)\n", what, a, b);
    abort();
}

namespace cv {

void fastFree(void *ptr) { free(ptr); }

void Mat::create(int d, const int *sizes, int _type) {
    if (d != 2 || sizes[0] < 0 || sizes[1] < 0) unsupported("create: dims / size", d, d == 2 ? sizes[0] : 0);
    _type &= TYPE_MASK;
    if (data && dims == 2 && rows == sizes[0] && cols == sizes[1] && type() == _type) return;
    release();
    const size_t esz = CV_ELEM_SIZE(_type);
    const size_t total = (size_t)sizes[0] * sizes[1] * esz;
    const size_t counter_at = (total + sizeof(int) - 1) / sizeof(int) * sizeof(int);
    uchar *block = (uchar *)malloc(counter_at + sizeof(int));     // the elements, then the reference counter
    if (!block) unsupported("create: out of memory", sizes[0], sizes[1]);
    flags = MAGIC_VAL | _type | CONTINUOUS_FLAG;
    dims = 2;
    rows = sizes[0];
    cols = sizes[1];
    step.p = step.buf;
    step.buf[0] = (size_t)cols * esz;
    step.buf[1] = esz;
    data = datastart = block;
    dataend = datalimit = block + total;
    refcount = (int *)(block + counter_at);
    *refcount = 1;
    allocator = 0;
}

void Mat::deallocate() {
    if (allocator) unsupported("deallocate: custom allocator", 0, 0);
    free(datastart);
}

Mat &Mat::operator=(const Scalar &s) {
    if (dims != 2) unsupported("fill: dims", dims, 0);
    const int cn = channels();
    if (depth() == CV_8U && cn >= 1 && cn <= 3) {
        uchar v[3];
        for (int c = 0; c < cn; c++) {
            if (s[c] != (double)(uchar)s[c]) unsupported("fill: value outside uchar", (int)s[c], c);
            v[c] = (uchar)s[c];
        }
        for (int y = 0; y < rows; y++) {
            uchar *p = data + step.buf[0] * y;
            for (int x = 0; x < cols; x++)
                for (int c = 0; c < cn; c++) p[x * cn + c] = v[c];
        }
    } else if (depth() == CV_16S && cn == 1) {
        if (s[0] != (double)(short)s[0]) unsupported("fill: value outside short", (int)s[0], 0);
        const short v = (short)s[0];
        for (int y = 0; y < rows; y++) {
            short *p = (short *)(data + step.buf[0] * y);
            for (int x = 0; x < cols; x++) p[x] = v;
        }
    } else {
        unsupported("fill: depth / channels", depth(), cn);
    }
    return *this;
}

}  // namespace cv
