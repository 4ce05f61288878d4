// Host harness of csrc/yf_box_term.h for tests/test_cpu_box_loss.py: reads records of 11 doubles (kind, t0..t3, aw, ah, tx, ty, gw, gh)
// from argv[1], writes 5 doubles each (value, d value / d t0..t3) to argv[2].  The same function the kernel calls, compiled for the host.
#include <stdio.h>

#include "yf_box_term.h"

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 3;
    double r[11], o[5];
    while (fread(r, sizeof(double), 11, in) == 11) {
        o[0] = yf::box_term((int)r[0], r + 1, r[5], r[6], r[7], r[8], r[9], r[10], o + 1);
        if (fwrite(o, sizeof(double), 5, out) != 5) return 4;
    }
    fclose(in);
    return fclose(out) ? 5 : 0;
}
