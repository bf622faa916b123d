// cw_witness — process-level drop-in for the reference's emitted calculator (SURVEY §8b seam 4):
//     reference:   ./<name> <input.json> <output.wtns>                 (main.cpp:336-373, <argv0>.dat beside it)
//     here:        cw_witness <name> <input.json> <output.wtns>        one instance, same files, same .wtns bytes
//                  cw_witness <name> <inputs.json> <out_%d.wtns>       inputs.json = JSON ARRAY of input objects:
//                                                                      one batch on the GPU, one .wtns per instance
//                  cw_witness --check <name> <a.wtns> [<b.wtns> ...]   witnesses IN (64-bit runtime): the files of any calculator
//                                                                      checked against <name>.r1cs in one batch, one line per
//                                                                      file: OK | MALFORMED | constraint <row> violated (+ the
//                                                                      wires by name when <name>.sym exists); exit 0 = all OK,
//                                                                      1 = some file is not, 2 = usage, I/O, another runtime
//                  cw_witness --sha256 <name> <input(s).json>           the same run, no file: one line per instance,
//                                                                      "<64 hex digits>  <instance index>", the SHA-256 of the
//                                                                      .wtns the plain call writes, computed on the device
//                                                                      (cw_get_wtns_digests); exit codes of the plain call
//                  cw_witness --compare <name> <input(s).json> <ref.wtns | ref_%d.wtns>
//                                                                      the same run, no file written: the .wtns of another
//                                                                      calculator compared byte by byte with what this batch
//                                                                      computes from the same inputs, on the device
//                                                                      (cw_compare_wtns_many); one line per instance, "instance
//                                                                      i: OK" | "instance i: entry k differs" (+ the signal's
//                                                                      name when <name>.sym exists); exit 0 = all equal, 1 = some
//                                                                      differ, 2 = usage, I/O (a file that is not the circuit's)
// <name> is the path prefix of <name>.cwt / <name>.dat / <name>.r1cs (the .r1cs is optional: without it the
// constraint check is skipped).  Exit code 0 = every instance produced a witness; 1 = at least one failed (the
// reference aborts on the first failed assert, calcwit/assert_bucket.rs:75-77; here the others are still written).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/circom_amd.h"
#include "cw_signals.h"

static std::string slurp(const char *path) {
    FILE *f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::string s;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, n);
    fclose(f);
    return s;
}

// split a top-level JSON array into the texts of its elements (objects); a top-level object is one element
static std::vector<std::string> elements(const std::string &t) {
    size_t i = 0;
    while (i < t.size() && isspace((unsigned char)t[i])) i++;
    if (i >= t.size() || t[i] != '[') return {t};
    std::vector<std::string> out;
    int depth = 0;
    bool in_str = false;
    size_t start = 0;
    for (; i < t.size(); i++) {
        char ch = t[i];
        if (in_str) {
            if (ch == '\\') i++;
            else if (ch == '"') in_str = false;
            continue;
        }
        if (ch == '"') in_str = true;
        else if (ch == '{' || ch == '[') {
            if (depth == 1 && ch == '{') start = i;
            depth++;
        } else if (ch == '}' || ch == ']') {
            depth--;
            if (depth == 1 && ch == '}') out.push_back(t.substr(start, i - start + 1));
            if (depth == 0) break;
        }
    }
    return out;
}

#define CHECK(call)                                                                      \
    do {                                                                                 \
        int rc_ = (call);                                                                \
        if (rc_ != CW_OK) { fprintf(stderr, "%s: %s\n", #call, cw_last_error()); return 2; } \
    } while (0)

// the batch counterpart of `snarkjs wtns check`: files[i] becomes instance i
static int check_files(const std::string &name, char **files, uint32_t n) {
    cw_circuit *c = nullptr;
    CHECK(cw_load((name + ".cwt").c_str(), (name + ".dat").c_str(), (name + ".r1cs").c_str(), &c));
    if (FILE *wl = fopen((name + ".w2s").c_str(), "rb")) {           // the witness list of a simplified system, as below
        std::vector<uint32_t> list;
        uint32_t v;
        while (fread(&v, 4, 1, wl) == 1) list.push_back(v);
        fclose(wl);
        if (!list.empty()) CHECK(cw_set_witness_list(c, list.data(), (uint32_t)list.size()));
    }
    const std::string sym = name + ".sym";
    FILE *sp = fopen(sym.c_str(), "rb");
    if (sp) fclose(sp);
    const int device = getenv("CW_DEVICE") ? atoi(getenv("CW_DEVICE")) : 0;
    cw_batch *b = nullptr;
    CHECK(cw_batch_create(c, device, n, nullptr, &b));
    for (uint32_t i = 0; i < n; i++) CHECK(cw_read_wtns(b, i, files[i]));
    CHECK(cw_check_r1cs(b));
    CHECK(cw_sync(b));
    std::vector<uint32_t> st(n), row(n);
    CHECK(cw_get_status(b, st.data()));
    CHECK(cw_get_r1cs_first_bad(b, row.data()));
    int bad = 0;
    std::vector<char> text(1 << 16);
    for (uint32_t i = 0; i < n; i++) {
        if (!st[i]) { printf("%s: OK\n", files[i]); continue; }
        bad++;
        if (st[i] & 8u) { printf("%s: MALFORMED\n", files[i]); continue; }
        printf("%s: constraint %u violated\n", files[i], row[i]);
        if (sp) {
            CHECK(cw_explain(b, i, sym.c_str(), text.data(), text.size()));
            fputs(text.data(), stdout);
        }
    }
    cw_batch_free(b);
    cw_free(c);
    return bad ? 1 : 0;
}

// the batch's own witnesses against the files of another calculator: ref (or ref % i) is compared with instance i
static int compare_files(const std::string &name, const char *input, const char *ref) {
    cw_circuit *c = nullptr;
    const std::string r1cs = name + ".r1cs";
    FILE *probe = fopen(r1cs.c_str(), "rb");
    if (probe) fclose(probe);
    CHECK(cw_load((name + ".cwt").c_str(), (name + ".dat").c_str(), probe ? r1cs.c_str() : nullptr, &c));
    std::vector<uint32_t> list;                                      // the witness list of a simplified system, as below
    if (FILE *wl = fopen((name + ".w2s").c_str(), "rb")) {
        uint32_t v;
        while (fread(&v, 4, 1, wl) == 1) list.push_back(v);
        fclose(wl);
        if (!list.empty()) CHECK(cw_set_witness_list(c, list.data(), (uint32_t)list.size()));
    }
    const std::vector<std::string> ins = elements(slurp(input));
    if (ins.empty()) { fprintf(stderr, "no input objects in %s\n", input); return 2; }
    const uint32_t n = (uint32_t)ins.size();
    // a pattern as the library's _many calls take it: a % (not %%), an optional width, then d or u
    bool many = false;
    for (const char *p = ref; *p && !many; p++)
        if (*p == '%') {
            if (p[1] == '%') { p++; continue; }
            const char *q = p + 1;
            while (*q >= '0' && *q <= '9') q++;
            many = *q == 'd' || *q == 'u';
        }
    if (!many && n > 1) { fprintf(stderr, "%u inputs need a reference pattern with %%d\n", n); return 2; }
    const int device = getenv("CW_DEVICE") ? atoi(getenv("CW_DEVICE")) : 0;
    cw_batch *b = nullptr;
    CHECK(cw_batch_create(c, device, n, nullptr, &b));
    for (uint32_t i = 0; i < n; i++) CHECK(cw_set_inputs_json(b, i, ins[i].c_str()));
    CHECK(cw_run(b));
    // verdicts are produced whatever the status word says; an instance whose run failed gets a line on stderr beside its verdict
    std::vector<uint32_t> st(n);
    CHECK(cw_get_status(b, st.data()));
    for (uint32_t i = 0; i < n; i++)
        if (st[i])
            fprintf(stderr, "instance %u: %s%s(its witness is compared as it stands)\n", i, (st[i] & 1) ? "Failed assert " : "",
                    (st[i] & 2) ? "division by zero " : "");
    std::vector<uint32_t> diff(n);
    uint32_t summary[2] = {0, 0};
    if (many) CHECK(cw_compare_wtns_many(b, 0, n, ref, diff.data(), summary));
    else CHECK(cw_compare_wtns(b, 0, ref, diff.data()));
    // entry k of the witness is signal list[k] of a simplified system and signal k otherwise (how this project's writers number
    // the witness); its name comes from <name>.sym through the walk cw_explain makes
    std::vector<std::string> names;
    {
        std::vector<uint8_t> buf;
        if (FILE *sp = fopen((name + ".sym").c_str(), "rb")) {
            char chunk[1 << 16];
            size_t got;
            while ((got = fread(chunk, 1, sizeof chunk, sp)) > 0) buf.insert(buf.end(), chunk, chunk + got);
            fclose(sp);
            names.assign(cw_n_signals(c), std::string());
            cwsig::sym_walk(buf, [&](unsigned long sid, const std::string &nm) {
                if (sid < names.size()) names[sid] = nm;
            });
        }
    }
    int differ = 0;
    for (uint32_t i = 0; i < n; i++) {
        if (diff[i] == 0xFFFFFFFFu) { printf("instance %u: OK\n", i); continue; }
        differ++;
        const uint32_t sid = list.empty() ? diff[i] : (diff[i] < list.size() ? list[diff[i]] : 0xFFFFFFFFu);
        if (sid == 0) printf("instance %u: entry %u differs (one)\n", i, diff[i]);
        else if (sid < names.size() && !names[sid].empty()) printf("instance %u: entry %u differs (%s)\n", i, diff[i], names[sid].c_str());
        else printf("instance %u: entry %u differs\n", i, diff[i]);
    }
    cw_batch_free(b);
    cw_free(c);
    return differ ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !strcmp(argv[1], "--compare")) {
        if (argc != 5) {
            fprintf(stderr, "Usage: %s --compare <circuit path prefix> <input(s).json> <ref.wtns | ref_%%d.wtns>\n", argv[0]);
            return 2;
        }
        return compare_files(argv[2], argv[3], argv[4]);
    }
    if (argc >= 2 && !strcmp(argv[1], "--check")) {
        if (argc < 4) {
            fprintf(stderr, "Usage: %s --check <circuit path prefix> <a.wtns> [<b.wtns> ...]\n", argv[0]);
            return 2;
        }
        return check_files(argv[2], argv + 3, (uint32_t)(argc - 3));
    }
    const bool sha = argc == 4 && !strcmp(argv[1], "--sha256");
    if (argc != 4) {
        fprintf(stderr, "Usage: %s <circuit path prefix> <input.json> <output.wtns | out_%%d.wtns>\n"
                        "       %s --sha256 <circuit path prefix> <input.json>\n"
                        "       %s --compare <circuit path prefix> <input(s).json> <ref.wtns | ref_%%d.wtns>\n", argv[0], argv[0], argv[0]);
        return 2;
    }
    const std::string name = sha ? argv[2] : argv[1];
    const char *input = sha ? argv[3] : argv[2];
    const std::string r1cs = name + ".r1cs";
    FILE *probe = fopen(r1cs.c_str(), "rb");
    if (probe) fclose(probe);
    cw_circuit *c = nullptr;
    CHECK(cw_load((name + ".cwt").c_str(), (name + ".dat").c_str(), probe ? r1cs.c_str() : nullptr, &c));
    // <name>.w2s beside the tape (written by `python -m circom_amd.circom` at its default level --O1): the signals the
    // simplified constraint system keeps, u32 little endian.  The files written below then hold THAT witness - what the
    // reference's calculator writes for the `.r1cs` it produced with the same flags.
    if (FILE *wl = fopen((name + ".w2s").c_str(), "rb")) {
        std::vector<uint32_t> list;
        uint32_t v;
        while (fread(&v, 4, 1, wl) == 1) list.push_back(v);
        fclose(wl);
        if (!list.empty()) CHECK(cw_set_witness_list(c, list.data(), (uint32_t)list.size()));
    }
    const std::vector<std::string> ins = elements(slurp(input));
    if (ins.empty()) { fprintf(stderr, "no input objects in %s\n", input); return 2; }
    const int device = getenv("CW_DEVICE") ? atoi(getenv("CW_DEVICE")) : 0;
    cw_batch *b = nullptr;
    CHECK(cw_batch_create(c, device, (uint32_t)ins.size(), nullptr, &b));
    for (size_t i = 0; i < ins.size(); i++) CHECK(cw_set_inputs_json(b, (uint32_t)i, ins[i].c_str()));
    CHECK(cw_run(b));
    if (probe) CHECK(cw_check_r1cs(b));
    CHECK(cw_sync(b));
    std::vector<uint32_t> st(ins.size());
    CHECK(cw_get_status(b, st.data()));
    int failed = 0;
    const bool many = !sha && strstr(argv[3], "%d") != nullptr;
    std::vector<uint8_t> digests(sha ? ins.size() * 32 : 0);
    if (sha) CHECK(cw_get_wtns_digests(b, 0, (uint32_t)ins.size(), digests.data()));
    if (!sha && !many && ins.size() > 1) { fprintf(stderr, "%zu inputs need an output pattern with %%d\n", ins.size()); return 2; }
    const bool logs = cw_n_log_statements(c) != 0;
    for (size_t i = 0; i < ins.size(); i++) {
        if (logs) {                 // what the reference binary prints for this input (log(...) statements), instance by instance
            const int64_t n = cw_get_log(b, (uint32_t)i, nullptr, 0);
            if (n < 0) { fprintf(stderr, "cw_get_log: %s\n", cw_last_error()); return 2; }
            std::vector<char> text((size_t)n + 1);
            if (cw_get_log(b, (uint32_t)i, text.data(), text.size()) < 0) { fprintf(stderr, "cw_get_log: %s\n", cw_last_error()); return 2; }
            fwrite(text.data(), 1, (size_t)n, stdout);
        }
        if (sha) {                  // every instance has a line: the digest is produced whatever the status word says
            for (int k = 0; k < 32; k++) printf("%02x", digests[i * 32 + k]);
            printf("  %zu\n", i);
        }
        if (st[i]) {
            fprintf(stderr, "instance %zu: %s%s%s\n", i, (st[i] & 1) ? "Failed assert " : "", (st[i] & 2) ? "division by zero " : "",
                    (st[i] & 4) ? "R1CS row violated" : "");
            failed++;
            continue;
        }
        if (sha) continue;
        char path[4096];
        if (many) snprintf(path, sizeof path, argv[3], (int)i);
        else snprintf(path, sizeof path, "%s", argv[3]);
        CHECK(cw_write_wtns(b, (uint32_t)i, path));
    }
    cw_batch_free(b);
    cw_free(c);
    return failed ? 1 : 0;
}
