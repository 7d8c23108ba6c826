// axis_pair_tree_check.cpp — a 64-lane model of the reductions of the axis-per-lane solve kernel (csrc/vigo_solver.hip):
// group_sum<32, 1>, the single tree that both halves of the wave run on the same operands, against pair_tree32<1>, which
// carries one sum in the lower half and another in the upper, and dot_xy against pack_xy.  The five cross-lane
// permutations are the ones the comment above dpp_f64 defines; every read is recorded, and a read that crosses the
// halves before the last exchange is an error.  Built by tests/test_axis_pair_tree.py with -O2 -ffp-contract=off.
// Prints "name value" lines; exit status 1 on any difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>

namespace {

constexpr int kWave = 64;
struct Wave {
    double v[kWave];
};
long long cross_reads = 0;   // reads of a lane of the other 32-lane half, inside the five tree levels

uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}
double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

// ---- the permutations ---------------------------------------------------------------------------------------------------
int quad_1032(int i) { return i ^ 1; }                          // quad_perm:[1,0,3,2]
int quad_2301(int i) { return i ^ 2; }                          // quad_perm:[2,3,0,1]
int row_half_mirror(int i) { return (i & ~7) | (7 - (i & 7)); }
int row_mirror(int i) { return (i & ~15) | (15 - (i & 15)); }

void note_read(int reader, int source) {
    if ((reader >> 5) != (source >> 5)) ++cross_reads;
}
Wave dpp(const Wave& a, int (*src)(int)) {
    Wave r;
    for (int i = 0; i < kWave; ++i) {
        note_read(i, src(i));
        r.v[i] = a.v[src(i)];
    }
    return r;
}
// v_permlane16_swap vdst, src: the odd rows of vdst and the even rows of src change places
void permlane16_swap(Wave& d, Wave& s) {
    for (int i = 0; i < kWave; ++i) {
        const int row = i >> 4;
        if (row & 1) {               // d's odd row <- s's even row below it, which receives d's odd row
            note_read(i, i - 16);
            note_read(i - 16, i);
            const double t = d.v[i];
            d.v[i] = s.v[i - 16];
            s.v[i - 16] = t;
        }
    }
}
// v_permlane32_swap vdst, src: the upper half of vdst and the lower half of src change places (the LAST exchange: free
// to cross the halves, that is what it is for)
void permlane32_swap(Wave& d, Wave& s) {
    for (int i = 32; i < kWave; ++i) {
        const double t = d.v[i];
        d.v[i] = s.v[i - 32];
        s.v[i - 32] = t;
    }
}
Wave add(const Wave& a, const Wave& b) {
    Wave r;
    for (int i = 0; i < kWave; ++i) r.v[i] = a.v[i] + b.v[i];
    return r;
}
Wave mul(const Wave& a, const Wave& b) {
    Wave r;
    for (int i = 0; i < kWave; ++i) r.v[i] = a.v[i] * b.v[i];
    return r;
}

// ---- the kernel's functions, statement for statement ----------------------------------------------------------------------
Wave levels_1_to_16(Wave v) {   // the five levels both trees share; returns p0 + p1
    v = add(v, dpp(v, quad_1032));
    v = add(v, dpp(v, quad_2301));
    v = add(v, dpp(v, row_half_mirror));
    const Wave t = dpp(v, row_mirror);
    Wave a = add(v, t), b = add(v, t);   // (the add and add_f64_again)
    permlane16_swap(a, b);               // xor16_parts: p0 = a, p1 = b
    return add(a, b);
}
Wave group_sum32(const Wave& v) { return levels_1_to_16(v); }
void pair_tree32(const Wave& v, Wave& lo, Wave& hi) {
    Wave a = levels_1_to_16(v), b = a;   // p0 + p1 and add_f64_again(p0, p1)
    permlane32_swap(a, b);               // xy_parts: x = a, y = b
    lo = a;
    hi = b;
}
Wave dot_xy(const Wave& p, const Wave& q) {
    Wave a = mul(p, q), b = a;           // (the product and mul_f64_again)
    permlane32_swap(a, b);
    return add(a, b);
}
Wave pack_xy(Wave u, Wave w) {
    permlane32_swap(u, w);
    return add(u, w);
}

// ---- inputs -------------------------------------------------------------------------------------------------------------
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}
double uniform() { return (double)(rnd() >> 11) * 0x1.0p-53 * 2.0 - 1.0; }
double special() {
    const double inf = std::numeric_limits<double>::infinity();
    switch (rnd() % 8) {
        case 0: return -0.0;
        case 1: return 0.0;
        case 2: return inf;
        case 3: return -inf;
        case 4: return std::numeric_limits<double>::quiet_NaN();
        case 5: return from_bits(rnd() & 0x000FFFFFFFFFFFFFull);                            // a denormal
        case 6: return -from_bits(rnd() & 0x000FFFFFFFFFFFFFull);
        default: return from_bits(0x7FF0000000000001ull | (rnd() & 0x8007FFFFFFFFFFFFull));   // a NaN with a payload
    }
}
// mode 0: ordinary values; 1: any bit pattern; 2: ordinary with specials among them; 3: zeros and denormals;
// 4: ordinary, the two sums hundreds of binades apart
double value(int mode, int half) {
    switch (mode) {
        case 0: return uniform() * 8.0;
        case 1: return from_bits(rnd());
        case 2: return rnd() % 16 == 0 ? special() : uniform();
        case 3: return rnd() % 4 == 0 ? (rnd() & 1 ? 0.0 : -0.0) : from_bits((rnd() & 0x000FFFFFFFFFFFFFull) | (rnd() << 63));
        default: return std::ldexp(uniform(), half ? 400 : -400);
    }
}

long long count_special = 0;
void census(double d) {
    if (!(std::fabs(d) <= std::numeric_limits<double>::max()) || d == 0.0 || std::fabs(d) < std::numeric_limits<double>::min())
        ++count_special;
}

}  // namespace

int main() {
    const int trials = 80000;   // x 64 lanes: 5.1 million packed inputs of the tree, as many pairs of products
    long long tree_diffs = 0, dot_diffs = 0, inputs = 0;
    for (int t = 0; t < trials; ++t) {
        const int mode = t % 5;
        Wave A, B, packed;   // A = [a | a], B = [b | b]: what the two single trees see; packed = [a | b]
        for (int l = 0; l < 32; ++l) {
            const double a = value(mode, 0), b = value(mode, 1);
            A.v[l] = A.v[l + 32] = a;
            B.v[l] = B.v[l + 32] = b;
            packed.v[l] = a;
            packed.v[l + 32] = b;
            census(a);
            census(b);
            inputs += 2;
        }
        cross_reads = 0;
        const Wave sa = group_sum32(A), sb = group_sum32(B);
        Wave lo, hi;
        pair_tree32(packed, lo, hi);
        if (cross_reads) {
            std::printf("cross_reads %lld\n", cross_reads);
            return 1;
        }
        for (int i = 0; i < kWave; ++i)
            if (bits(lo.v[i]) != bits(sa.v[i]) || bits(hi.v[i]) != bits(sb.v[i])) ++tree_diffs;

        // two dot products of per-lane coordinates (p . q and p . r), as dot_xy twice and as pack_xy of the products
        Wave p, q, r;
        for (int i = 0; i < kWave; ++i) {
            p.v[i] = value(mode, 0);
            q.v[i] = value(mode, 1);
            r.v[i] = value(mode, 0);
        }
        const Wave d1 = dot_xy(p, q), d2 = dot_xy(p, r), pk = pack_xy(mul(p, q), mul(p, r));
        for (int i = 0; i < kWave; ++i)
            if (bits(pk.v[i]) != bits(i < 32 ? d1.v[i] : d2.v[i])) ++dot_diffs;
    }
    std::printf("trials %d\ninputs %lld\nspecial_inputs %lld\ncross_reads 0\ntree_diffs %lld\ndot_diffs %lld\n", trials, inputs,
                count_special, tree_diffs, dot_diffs);
    return tree_diffs || dot_diffs ? 1 : 0;
}
