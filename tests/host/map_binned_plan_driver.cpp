// map_binned_plan_driver.cpp -- clc_map_binned_plan without a device, for tests/test_map_binned_abi.py: the plan reads nothing of a
// context but the number of its map rows, so a default-constructed clc_ctx (no device, no allocation) with map_n set stands in for one.
// usage: map_binned_plan_driver <cases.txt>   each line "ppx ppy radius_bits map_n" (doubles as hex floats, the radius as the uint32 bits
// of the float); prints per line "rc plan cells lanes zero cell_side" (cell_side as a hex float).
#include <cstdio>
#include <cstring>

#include "clc_ctx.h"

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    clc_ctx ctx;
    double ppx, ppy;
    unsigned bits;
    long map_n;
    while (std::fscanf(f, "%la %la %x %ld", &ppx, &ppy, &bits, &map_n) == 4) {
        float radius;
        std::memcpy(&radius, &bits, 4);
        ctx.map_n = (int)map_n;
        const clc_camera_k3 cam{ 500.0, ppx, ppy, 0.0, 0.0, 0.0 };
        int32_t info[4] = { -9, -9, -9, -9 };
        double side = -1.0;
        const int rc = clc_map_binned_plan(&ctx, &cam, radius, info, &side);
        std::printf("%d %d %d %d %d %a\n", rc, info[0], info[1], info[2], info[3], side);
    }
    std::fclose(f);
    return 0;
}
