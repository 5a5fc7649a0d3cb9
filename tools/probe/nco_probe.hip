// gfx950 latency probe for the exact-oscillator chain (k_nco_exact): one float complex multiplication per step, every step dependent on the last.
//   hipcc tools/probe/nco_probe.hip -o gpurun_out/nco_probe --offload-arch=gfx950 -O3 -ffp-contract=off && gpurun_out/nco_probe
// Part 1 (round 6), the bare chain without a table: packed (2 v_pk_mul_f32 + 1 v_pk_add_f32), scalar (4 v_mul_f32 + v_sub_f32 + v_add_f32), two lanes per
// chain with the partner's component through DPP (2 v_mul_f32_dpp + 1 v_add_f32 + the wait states a DPP read of a fresh VALU result needs).
// Part 2 (round 7), the kernel's shape -- 32 symbols of 2160 steps, renormalised after each, EVERY step's phasor left in a table -- in the forms of
// getting the phasors out of the chain's registers: the tables of all forms must be equal byte for byte (checked against form 0).
//   0 lane0     one lane works and stores 8 bytes per step (round 6's kernel)
//   1 select    all 64 lanes run the chain; lane j & 63 keeps step j's phasor by two v_cndmask_b32 on a one-bit mask in an SGPR pair; a 512-byte row per 64 steps
//   2 select-c  the same with the selects left to the compiler (v_cmp_eq + 2 v_cndmask_b32)
//   3 execmov   ... kept by one v_mov_b64 under EXEC = the one-bit mask
//   4 freeze    EXEC loses one lane per step (s_lshl_b64 exec, exec, 1), so lane l stops on step l's phasor: no instruction beside the chain's three and the shift;
//               once per row lane 63's phasor goes back to all lanes (v_readlane_b32)
//   5 freeze-s  form 4 on the six plain instructions
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
typedef float cf __attribute__((ext_vector_type(2)));
constexpr int STEPS = 69120, NSYM = 32, SYM_N = 2160;

__global__ __launch_bounds__(64) void k_packed(float2 *out, float c, float d)
{
    if (threadIdx.x) return;
    cf P = {1.0f, 0.0f}; const cf K = {c, d};
#pragma unroll 8
    for (int j = 0; j < STEPS; j++) {
        cf t1, t2;
        asm("v_pk_mul_f32 %1, %0, %3 op_sel_hi:[0,1]\n\tv_pk_mul_f32 %2, %0, %3 op_sel:[1,1] op_sel_hi:[1,0]\n\tv_pk_add_f32 %0, %1, %2 neg_lo:[0,1]" : "+v"(P), "=&v"(t1), "=&v"(t2) : "v"(K));
    }
    out[blockIdx.x] = make_float2(P.x, P.y);
}
__global__ __launch_bounds__(64) void k_scalar(float2 *out, float c, float d)
{
    if (threadIdx.x) return;
    float a = 1.0f, b = 0.0f;
#pragma unroll 8
    for (int j = 0; j < STEPS; j++) {
        float ac, bd, ad, bc;
        asm("v_mul_f32 %2, %0, %6\n\tv_mul_f32 %3, %1, %7\n\tv_mul_f32 %4, %0, %7\n\tv_mul_f32 %5, %1, %6\n\tv_sub_f32 %0, %2, %3\n\tv_add_f32 %1, %4, %5"
            : "+v"(a), "+v"(b), "=&v"(ac), "=&v"(bd), "=&v"(ad), "=&v"(bc) : "v"(c), "v"(d));
    }
    out[blockIdx.x] = make_float2(a, b);
}
// lanes 0 / 1 of a quad: r = re in lane 0, im in lane 1.  k1 = (c, d), k2 = (-d, c) per lane: lane 0: a c + b (-d), lane 1: a d + b c
template <int NOP>
__global__ __launch_bounds__(64) void k_dpp(float2 *out, float c, float d)
{
    if (threadIdx.x > 1) return;
    float r = threadIdx.x == 0 ? 1.0f : 0.0f;
    const float k1 = threadIdx.x == 0 ? c : d, k2 = threadIdx.x == 0 ? -d : c;
#pragma unroll 8
    for (int j = 0; j < STEPS; j++) {
        float t1, t2;
        if (NOP == 1)
            asm("s_nop 1\n\tv_mul_f32_dpp %1, %0, %3 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\tv_mul_f32_dpp %2, %0, %4 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32 %0, %1, %2"
                : "+v"(r), "=&v"(t1), "=&v"(t2) : "v"(k1), "v"(k2));
        else
            asm("s_nop 0\n\tv_mul_f32_dpp %1, %0, %3 quad_perm:[0,0,0,0] row_mask:0xf bank_mask:0xf\n\tv_mul_f32_dpp %2, %0, %4 quad_perm:[1,1,1,1] row_mask:0xf bank_mask:0xf\n\tv_add_f32 %0, %1, %2"
                : "+v"(r), "=&v"(t1), "=&v"(t2) : "v"(k1), "v"(k2));
    }
    if (threadIdx.x == 0) out[blockIdx.x].x = r; else out[blockIdx.x].y = r;
}

template <typename K> static void run(K kern, const char *name, float2 *out, int nblocks)
{
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    const float c = 0.99999976f, d = 6.9e-4f;
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), 0, 0, out, c, d);
    hipDeviceSynchronize();
    hipEventRecord(a, 0);
    for (int r = 0; r < 5; r++) hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), 0, 0, out, c, d);
    hipEventRecord(b, 0); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    float2 h; hipMemcpy(&h, out, sizeof(h), hipMemcpyDeviceToHost);
    printf("%-10s blocks %4d: %8.3f ms per launch = %6.2f ns per step   result (%.9g, %.9g)\n", name, nblocks, ms / 5, ms / 5 * 1e6 / STEPS, h.x, h.y);
}

// ---- part 2 ---------------------------------------------------------------------------------------------------------------------------------
#define PK_STEP "v_pk_mul_f32 %[t1], %[p], %[k] op_sel_hi:[0,1]\n\tv_pk_mul_f32 %[t2], %[p], %[k] op_sel:[1,1] op_sel_hi:[1,0]\n\t"
#define PK_ADD "v_pk_add_f32 %[p], %[t1], %[t2] neg_lo:[0,1]"
#define PK_OPS [p] "+v"(P), [t1] "=&v"(t1), [t2] "=&v"(t2)

// R steps of a row with the phasor of step u left in lane u (u < R); P: the phasor in front of the row in, the one behind it out (all lanes)
template <int FORM, int R> __device__ __forceinline__ cf row_steps(cf &P, const cf K, int lane)
{
    cf keep = P, t1, t2;
    if (FORM == 1) {
        unsigned long long mask = 1;
        float kx = P.x, ky = P.y;
#pragma unroll 8
        for (int u = 0; u < R; u++) {
            asm("v_cndmask_b32_e64 %0, %0, %2, %4\n\tv_cndmask_b32_e64 %1, %1, %3, %4" : "+v"(kx), "+v"(ky) : "v"(P.x), "v"(P.y), "s"(mask));
            asm(PK_STEP PK_ADD : PK_OPS : [k] "v"(K));
            mask <<= 1;
        }
        keep.x = kx; keep.y = ky;
    } else if (FORM == 2) {
#pragma unroll 8
        for (int u = 0; u < R; u++) {
            keep = lane == u ? P : keep;
            asm(PK_STEP PK_ADD : PK_OPS : [k] "v"(K));
        }
    }
    return keep;
}

template <int FORM> __global__ __launch_bounds__(64) void k_table(float2 *tabs, float2 *last, float c, float d)
{
    const int lane = threadIdx.x;
    if (FORM == 0 && lane != 0) return;
    float pr = 1.25f, pi = 0.0f;                               // a start phasor of magnitude != 1: the first renormalisation does something
    float2 *tab = tabs + (size_t)blockIdx.x * NSYM * SYM_N;
    const cf K = {c, d};
    for (int sym = 0; sym < NSYM; sym++) {
        cf P = {pr, pi};
        cf *out = (cf *)(tab + sym * SYM_N);
        if (FORM == 0) {
#pragma unroll 8
            for (int j = 0; j < SYM_N; j++) {
                out[j] = P;
                cf t1, t2;
                asm(PK_STEP PK_ADD : PK_OPS : [k] "v"(K));
            }
        } else if (FORM == 1 || FORM == 2) {
            for (int row = 0; row < SYM_N / 64; row++) { const cf keep = row_steps<FORM, 64>(P, K, lane); out[row * 64 + lane] = keep; }
            const cf keep = row_steps<FORM, SYM_N % 64>(P, K, lane);
            if (lane < SYM_N % 64) out[(SYM_N / 64) * 64 + lane] = keep;
        } else if (FORM == 3) {
            for (int row = 0; row <= SYM_N / 64; row++) {
                const int R = row < SYM_N / 64 ? 64 : SYM_N % 64;
                unsigned long long mask = 1;
                cf keep = P, t1, t2;
#pragma unroll 8
                for (int u = 0; u < R; u++)
                    asm(PK_STEP "s_mov_b64 exec, %[m]\n\tv_mov_b64 %[keep], %[p]\n\ts_mov_b64 exec, -1\n\ts_lshl_b64 %[m], %[m], 1\n\t" PK_ADD
                        : PK_OPS, [keep] "+v"(keep), [m] "+s"(mask) : [k] "v"(K) : "scc");
                if (lane < R) out[row * 64 + lane] = keep;
            }
        } else {
            // EXEC shrinks by one lane per step: lane l takes part in the first l steps of the row.  The whole row is ONE statement: between two statements
            // the compiler may place instructions of its own, which must not run under a partial EXEC
            for (int row = 0; row <= SYM_N / 64; row++) {
                const int R = row < SYM_N / 64 ? 64 : SYM_N % 64;
                if (FORM == 4) {
                    cf t1, t2;
                    if (R == 64) asm volatile(".rept 63\n\ts_lshl_b64 exec, exec, 1\n\t" PK_STEP PK_ADD "\n\t.endr\n\ts_mov_b64 exec, -1" : PK_OPS : [k] "v"(K) : "scc");
                    else asm volatile(".rept 47\n\ts_lshl_b64 exec, exec, 1\n\t" PK_STEP PK_ADD "\n\t.endr\n\ts_mov_b64 exec, -1" : PK_OPS : [k] "v"(K) : "scc");
                } else {
                    float a = P.x, b = P.y, ac, bd, ad, bc;
#define SC_STEP "v_mul_f32 %2, %0, %6\n\tv_mul_f32 %3, %1, %7\n\tv_mul_f32 %4, %0, %7\n\tv_mul_f32 %5, %1, %6\n\tv_sub_f32 %0, %2, %3\n\tv_add_f32 %1, %4, %5"
                    if (R == 64) asm volatile(".rept 63\n\ts_lshl_b64 exec, exec, 1\n\t" SC_STEP "\n\t.endr\n\ts_mov_b64 exec, -1" : "+v"(a), "+v"(b), "=&v"(ac), "=&v"(bd), "=&v"(ad), "=&v"(bc) : "v"(c), "v"(d) : "scc");
                    else asm volatile(".rept 47\n\ts_lshl_b64 exec, exec, 1\n\t" SC_STEP "\n\t.endr\n\ts_mov_b64 exec, -1" : "+v"(a), "+v"(b), "=&v"(ac), "=&v"(bd), "=&v"(ad), "=&v"(bc) : "v"(c), "v"(d) : "scc");
                    P.x = a; P.y = b;
                }
                if (lane < R) out[row * 64 + lane] = P;
                // the last lane's phasor to every lane, then the row's last step by all of them
                const float lx = P.x, ly = P.y;                // (through plain floats: a bit cast applied to P.y directly read P.x)
                P.x = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(lx), R - 1));
                P.y = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ly), R - 1));
                cf t1, t2;
                asm(PK_STEP PK_ADD : PK_OPS : [k] "v"(K));
            }
        }
        pr = P.x; pi = P.y;
        const float m = (float)sqrt((double)pr * (double)pr + (double)pi * (double)pi);
        pr = pr / m; pi = pi / m;
    }
    if (lane == 0) last[blockIdx.x] = make_float2(pr, pi);
}

template <typename K> static float run_table(K kern, const char *name, float2 *tabs, float2 *last, int nblocks, std::vector<float2> &host)
{
    hipEvent_t a, b; hipEventCreate(&a); hipEventCreate(&b);
    const float c = 0.99999976f, d = 6.9e-4f;
    const size_t n = (size_t)nblocks * NSYM * SYM_N;
    hipMemset(tabs, 0xA5, n * sizeof(float2));
    hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), 0, 0, tabs, last, c, d);
    if (hipDeviceSynchronize() != hipSuccess) { printf("%-10s FAILED: %s\n", name, hipGetErrorString(hipGetLastError())); exit(1); }
    hipEventRecord(a, 0);
    for (int r = 0; r < 5; r++) hipLaunchKernelGGL(kern, dim3(nblocks), dim3(64), 0, 0, tabs, last, c, d);
    hipEventRecord(b, 0); hipEventSynchronize(b);
    float ms = 0; hipEventElapsedTime(&ms, a, b);
    host.resize(n + nblocks);
    hipMemcpy(host.data(), tabs, n * sizeof(float2), hipMemcpyDeviceToHost);
    hipMemcpy(host.data() + n, last, nblocks * sizeof(float2), hipMemcpyDeviceToHost);
    printf("%-10s blocks %4d: %8.3f ms per launch = %6.2f ns per step   end (%.9g, %.9g)\n", name, nblocks, ms / 5, ms / 5 * 1e6 / STEPS, host[n].x, host[n].y);
    return ms / 5;
}

int main(int argc, char **argv)
{
    float2 *out; hipMalloc(&out, 4096 * sizeof(float2));
    if (argc < 2)
        for (int nb : {1, 256, 2048}) {
            run(k_packed, "packed", out, nb);
            run(k_scalar, "scalar", out, nb);
            run(k_dpp<1>, "dpp nop1", out, nb);
            run(k_dpp<0>, "dpp nop0", out, nb);
        }
    int bad = 0;
    for (int nb : {1, 256}) {
        float2 *tabs; hipMalloc(&tabs, (size_t)nb * NSYM * SYM_N * sizeof(float2));
        std::vector<float2> ref, got;
        run_table(k_table<0>, "lane0", tabs, out, nb, ref);
        const char *names[5] = {"select", "select-c", "execmov", "freeze", "freeze-s"};
        for (int f = 1; f <= 5; f++) {
            switch (f) {
            case 1: run_table(k_table<1>, names[0], tabs, out, nb, got); break;
            case 2: run_table(k_table<2>, names[1], tabs, out, nb, got); break;
            case 3: run_table(k_table<3>, names[2], tabs, out, nb, got); break;
            case 4: run_table(k_table<4>, names[3], tabs, out, nb, got); break;
            default: run_table(k_table<5>, names[4], tabs, out, nb, got); break;
            }
            const bool same = got.size() == ref.size() && memcmp(got.data(), ref.data(), ref.size() * sizeof(float2)) == 0;
            printf("    %s: table and end phasor %s form 0's\n", names[f - 1], same ? "EQUAL" : "DIFFER FROM");
            bad += !same;
        }
        hipFree(tabs);
    }
    return bad ? 1 : 0;
}
