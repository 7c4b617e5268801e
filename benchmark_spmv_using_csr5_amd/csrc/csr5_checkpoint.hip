// csr5_checkpoint.hip -- serialise / deserialise (checkpoint of the converted matrix)
// File = header + row_ptr + column_index and value IN TILE ORDER + the four CSR5 arrays of the reference
// (anonymouslib_cuda.h:27-52).  Loading skips the conversion: only the kernel-side tables are re-derived.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "csr5_handle.h"

using namespace csr5;

extern "C" { // (from here on, as the unit this came from had it: the two file helpers keep the names they have in the library's symbol table)

namespace {
struct Csr5FileHeader {
    char magic[8];      // "CSR5HIP1"
    int32_t value_type, omega, sigma, m, n, nnz, p, num_packet, num_offsets, tail_start;
    int32_t reserved[4];
};
bool write_dev(FILE *f, const void *dptr, size_t bytes, std::vector<char> &stage)
{
    if (!bytes)
        return true;
    stage.resize(bytes);
    if (hipMemcpy(stage.data(), dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess)
        return false;
    return fwrite(stage.data(), 1, bytes, f) == bytes;
}
bool read_dev(FILE *f, void *dptr, size_t bytes, std::vector<char> &stage)
{
    if (!bytes)
        return true;
    stage.resize(bytes);
    if (fread(stage.data(), 1, bytes, f) != bytes)
        return false;
    return hipMemcpy(dptr, stage.data(), bytes, hipMemcpyHostToDevice) == hipSuccess;
}
} // namespace

int csr5hip_save(csr5hip_handle h, const char *path)
{
    if (!h || !path)
        return CSR5HIP_INVALID_ARGUMENT;
    if (h->format != CSR5HIP_FORMAT_CSR5) {
        set_last_error("csr5hip_save: the handle is not in CSR5 format");
        return CSR5HIP_UNKOWN_FORMAT;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    FILE *f = fopen(path, "wb");
    if (!f) {
        set_last_error(std::string("csr5hip_save: cannot open ") + path);
        return CSR5HIP_INVALID_ARGUMENT;
    }
    const Geometry &g = h->g;
    Csr5FileHeader hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.magic, "CSR5HIP1", 8);
    hd.value_type = h->value_type, hd.omega = OMEGA, hd.sigma = g.sigma, hd.m = g.m, hd.n = g.n, hd.nnz = g.nnz;
    hd.p = g.p, hd.num_packet = g.num_packet, hd.num_offsets = h->num_offsets, hd.tail_start = g.tail_start;
    std::vector<char> stage;
    bool ok = fwrite(&hd, sizeof hd, 1, f) == 1;
    ok = ok && write_dev(f, h->d.row_ptr, ((size_t)g.m + 1) * 4, stage);
    ok = ok && write_dev(f, h->d.col, (size_t)g.nnz * 4, stage);
    ok = ok && write_dev(f, h->d.val, (size_t)g.nnz * h->vsize(), stage);
    ok = ok && write_dev(f, h->d.tile_ptr, ((size_t)g.p + 1) * 4, stage);
    ok = ok && write_dev(f, h->d.tile_desc, (size_t)g.p * OMEGA * g.num_packet * 4, stage);
    ok = ok && write_dev(f, h->d.offset_ptr, ((size_t)g.p + 1) * 4, stage);
    ok = ok && write_dev(f, h->d.offset, (size_t)h->num_offsets * 4, stage);
    ok = (fclose(f) == 0) && ok;
    if (!ok) {
        set_last_error(std::string("csr5hip_save: write failed: ") + path);
        return CSR5HIP_HIP_ERROR;
    }
    return CSR5HIP_SUCCESS;
}

int csr5hip_load(const char *path, csr5hip_handle *out, csr5hip_csr *arrays)
{
    if (!path || !out || !arrays)
        return CSR5HIP_INVALID_ARGUMENT;
    *out = nullptr;
    memset(arrays, 0, sizeof *arrays);
    FILE *f = fopen(path, "rb");
    if (!f) {
        set_last_error(std::string("csr5hip_load: cannot open ") + path);
        return CSR5HIP_INVALID_ARGUMENT;
    }
    Csr5FileHeader hd;
    bool ok = fread(&hd, sizeof hd, 1, f) == 1 && memcmp(hd.magic, "CSR5HIP1", 8) == 0;
    ok = ok && hd.omega == OMEGA && (hd.value_type == CSR5HIP_F64 || hd.value_type == CSR5HIP_F32);
    ok = ok && hd.m >= 0 && hd.n >= 0 && hd.nnz >= 0 && hd.sigma >= CSR5HIP_MIN_SIGMA && hd.sigma <= CSR5HIP_MAX_SIGMA;
    ok = ok && hd.num_offsets >= 0 && hd.tail_start >= 0 && hd.tail_start <= hd.m;
    ok = ok && hd.p == (int)(((long long)hd.nnz + (long long)OMEGA * hd.sigma - 1) / ((long long)OMEGA * hd.sigma));
    ok = ok && hd.num_packet == num_packet_of(hd.sigma);
    if (!ok) {
        fclose(f);
        set_last_error(std::string("csr5hip_load: not a CSR5 checkpoint of this library: ") + path);
        return CSR5HIP_INVALID_ARGUMENT;
    }
    const size_t vs = hd.value_type == CSR5HIP_F64 ? 8 : 4;
    // the file must be exactly as long as its header implies (a truncated or padded file is rejected before any
    // nnz-sized allocation)
    {
        const long long expect = (long long)sizeof hd + ((long long)hd.m + 1) * 4 + (long long)hd.nnz * (4 + (long long)vs) +
                                 ((long long)hd.p + 1) * 8 + (long long)hd.p * OMEGA * hd.num_packet * 4 +
                                 (long long)hd.num_offsets * 4;
        long long have = -1;
        const long pos = ftell(f);
        if (pos >= 0 && fseek(f, 0, SEEK_END) == 0) {
            have = ftell(f);
            if (fseek(f, pos, SEEK_SET) != 0)
                have = -1;
        }
        if (have != expect) {
            fclose(f);
            set_last_error(std::string("csr5hip_load: file size does not match its header: ") + path);
            return CSR5HIP_INVALID_ARGUMENT;
        }
    }
    csr5hip_handle h = nullptr;
    int rc = csr5hip_create(&h, hd.m, hd.n, hd.value_type);
    auto fail_with = [&](int code, const char *msg) {
        if (msg)
            set_last_error(std::string("csr5hip_load: ") + msg);
        fclose(f);
        if (h)
            csr5hip_free(h);
        csr5hip_csr_release(arrays);
        return code;
    };
    if (rc != CSR5HIP_SUCCESS)
        return fail_with(rc, nullptr);
    arrays->m = hd.m, arrays->n = hd.n, arrays->nnz = hd.nnz, arrays->value_type = hd.value_type;
    if (hipMalloc(&arrays->d_row_ptr, ((size_t)hd.m + 1) * 4) != hipSuccess ||
        hipMalloc(&arrays->d_col_idx, (size_t)(hd.nnz ? hd.nnz : 1) * 4) != hipSuccess ||
        hipMalloc(&arrays->d_val, (size_t)(hd.nnz ? hd.nnz : 1) * vs) != hipSuccess)
        return fail_with(CSR5HIP_HIP_ERROR, "device allocation failed");
    std::vector<char> stage;
    ok = read_dev(f, arrays->d_row_ptr, ((size_t)hd.m + 1) * 4, stage);
    ok = ok && read_dev(f, arrays->d_col_idx, (size_t)hd.nnz * 4, stage);
    ok = ok && read_dev(f, arrays->d_val, (size_t)hd.nnz * vs, stage);
    if (!ok)
        return fail_with(CSR5HIP_INVALID_ARGUMENT, "truncated file");
    csr5hip_input_csr(h, hd.nnz, arrays->d_row_ptr, arrays->d_col_idx, arrays->d_val);
    h->sigma_request = hd.sigma;
    h->sigma_auto = false;
    rc = derive_geometry(h, hd.sigma);
    if (rc == CSR5HIP_SUCCESS)
        rc = reserve_aux(h);
    if (rc != CSR5HIP_SUCCESS)
        return fail_with(rc, nullptr);
    // row_ptr and column_index are used as addresses by every kernel: check them on the device before anything
    // reads through them (row_ptr monotone from 0 to nnz, columns inside [0, n))
    {
        uint32_t bad = 0;
        hipError_t e = hipMemsetAsync(h->d.counters, 0, 16, h->stream);
        if (e == hipSuccess)
            e = launch_validate_csr(hd.m, hd.n, hd.nnz, arrays->d_row_ptr, arrays->d_col_idx, h->d.counters, h->stream);
        if (e == hipSuccess)
            e = hipMemcpyAsync(&bad, h->d.counters, 4, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream);
        if (e == hipSuccess)
            e = hipMemsetAsync(h->d.counters, 0, 16, h->stream);
        if (e != hipSuccess)
            return fail_with(fail_hip(e, "csr5hip_load: validation"), nullptr);
        if (bad)
            return fail_with(CSR5HIP_INVALID_ARGUMENT, bad & 1u ? "row_ptr is not a monotone pointer array ending at nnz"
                                                                 : "a column index lies outside [0, n)");
    }
    // The four format arrays are a pure function of row_ptr and sigma: they are RE-DERIVED here (cheap: no transpose)
    // and the file's copies only have to match -- nothing read from the file is ever used as an index unchecked.
    if (hd.p > 0) {
        rc = build_format_arrays(h);
        if (rc != CSR5HIP_SUCCESS)
            return fail_with(rc, nullptr);
        if (read_format_scalars(h, true) != hipSuccess)
            return fail_with(CSR5HIP_HIP_ERROR, "reading the conversion scalars failed");
        finish_format_scalars(h);
        if (h->g.tail_start != hd.tail_start || h->num_offsets != hd.num_offsets)
            return fail_with(CSR5HIP_INVALID_ARGUMENT, "format arrays do not belong to this row_ptr (tail start / offsets)");
    } else if (hd.num_offsets != 0) {
        return fail_with(CSR5HIP_INVALID_ARGUMENT, "format arrays do not belong to this row_ptr");
    }
    {
        std::vector<char> mine;
        auto same = [&](const void *dptr, size_t bytes) -> bool {
            if (!bytes)
                return true;
            stage.resize(bytes);
            mine.resize(bytes);
            if (fread(stage.data(), 1, bytes, f) != bytes)
                return false;
            if (hipMemcpy(mine.data(), dptr, bytes, hipMemcpyDeviceToHost) != hipSuccess)
                return false;
            return memcmp(stage.data(), mine.data(), bytes) == 0;
        };
        ok = same(h->d.tile_ptr, ((size_t)hd.p + 1) * 4);
        ok = ok && same(h->d.tile_desc, (size_t)hd.p * OMEGA * hd.num_packet * 4);
        ok = ok && same(h->d.offset_ptr, ((size_t)hd.p + 1) * 4);
        ok = ok && same(h->d.offset, (size_t)hd.num_offsets * 4);
        if (!ok)
            return fail_with(CSR5HIP_INVALID_ARGUMENT, "format arrays in the file do not match the ones derived from its row_ptr");
    }
    if (hd.p > 0) {
        rc = derive_kernel_tables(h);
        if (rc != CSR5HIP_SUCCESS)
            return fail_with(rc, nullptr);
    }
    fclose(f);
    resolve_variants(h);
    h->format = CSR5HIP_FORMAT_CSR5;
    rc = build_slabs(h); // (ends with prepare_plain when the plain path serves spmv())
    if (rc != CSR5HIP_SUCCESS) {
        csr5hip_free(h);
        csr5hip_csr_release(arrays);
        return rc;
    }
    *out = h;
    return CSR5HIP_SUCCESS;
}

} // extern "C"
