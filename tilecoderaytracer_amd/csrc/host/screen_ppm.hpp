/*
 * screen_ppm.hpp -- writer for a binary PPM (netpbm P6), the plainest file an image viewer opens: "P6\n<W> <H>\n255\n", then H
 * rows of 3 W bytes r, g, b, top row first -- the rows rt_encode_image (include/rt_capi_image.h) makes with 3 channels and
 * bottom_up 0.  In memory the rows may lie pitch_bytes >= 3 W apart; the file's rows are dense.
 */
#ifndef SCREEN_PPM_HPP_
#define SCREEN_PPM_HPP_

#include <cstddef>
#include <cstdint>
#include <cstdio>

/* returns 0 ok / 1 error, like celio_write_screen_txt */
inline int celio_write_screen_ppm(const char *path, int W, int H, const uint8_t *rows, uint64_t pitch_bytes) {
    if (!path || !rows || W <= 0 || H <= 0 || pitch_bytes < (uint64_t)W * 3u) return 1;
    std::FILE *f = std::fopen(path, "wb");
    if (!f) {
        std::printf("Error Opening File %s\n", path);
        return 1;
    }
    int rc = std::fprintf(f, "P6\n%d %d\n255\n", W, H) < 0 ? 1 : 0;
    const size_t row_bytes = (size_t)W * 3u;
    if (pitch_bytes == row_bytes) {
        if (std::fwrite(rows, row_bytes, (size_t)H, f) != (size_t)H) rc = 1;
    } else {
        for (int r = 0; r < H && !rc; ++r)
            if (std::fwrite(rows + (size_t)r * pitch_bytes, 1, row_bytes, f) != row_bytes) rc = 1;
    }
    if (std::fclose(f)) rc = 1;
    return rc;
}

#endif /* SCREEN_PPM_HPP_ */
