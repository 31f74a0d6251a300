// Host-only pieces of the scoring interface: the text model file
// ("COCOA-MODEL 1") and the classification-error rule on decision values.
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/cocoa_capi.h"
#include "common.h"
#include "jdouble.h"

namespace {

int fail(int code, const std::string& msg) {
    cocoa_set_global_error(msg);
    return code;
}

// one line without its terminator ('\n' or "\r\n"); false at end of file
bool next_line(const std::string& s, size_t& pos, std::string& line) {
    if (pos >= s.size()) return false;
    size_t e = s.find('\n', pos);
    if (e == std::string::npos) e = s.size();
    line.assign(s, pos, e - pos);
    if (!line.empty() && line.back() == '\r') line.pop_back();
    pos = e + 1;
    return true;
}

// Double.toString spellings back to the double they came from: glibc's strtod
// rounds correctly, and Java's "NaN" / "Infinity" / "-Infinity" are spelled out
bool parse_double(const std::string& t, double& out) {
    if (t.empty() || t[0] == ' ' || t[0] == '\t') return false;
    if (t == "NaN") {
        out = std::nan("");
        return true;
    }
    if (t == "Infinity" || t == "-Infinity") {
        out = t[0] == '-' ? -INFINITY : INFINITY;
        return true;
    }
    for (char c : t)
        if (!((c >= '0' && c <= '9') || c == '-' || c == '+' || c == '.' || c == 'E' || c == 'e')) return false;
    char* e = nullptr;
    errno = 0;
    out = std::strtod(t.c_str(), &e);
    return e != t.c_str() && *e == 0;
}

bool parse_field(const std::string& line, const char* key, std::string& value) {
    const size_t k = std::strlen(key);
    if (line.compare(0, k, key) != 0 || line.size() <= k || line[k] != ' ') return false;
    value = line.substr(k + 1);
    return true;
}

}  // namespace

extern "C" int cocoa_score_errors(const double* f, const double* y, int64_t n_rows, int64_t* err_count) {
    if (n_rows < 0 || !err_count || (n_rows > 0 && (!f || !y))) return fail(COCOA_E_ARG, "cocoa_score_errors: bad argument");
    int64_t err = 0;
    for (int64_t r = 0; r < n_rows; ++r)
        if (!(f[r] * y[r] > 0.0)) ++err;  // OptUtils.scala:95-98 (a NaN or zero score is an error)
    *err_count = err;
    return COCOA_OK;
}

extern "C" int cocoa_model_save(const char* path, const double* w, int32_t num_features, const char* method,
                                double lambda, int32_t rounds) {
    if (!path || !w || num_features < 1) return fail(COCOA_E_ARG, "cocoa_model_save: bad argument");
    std::string name = method && *method ? method : "unknown";
    for (char c : name)
        if (c == '\n' || c == '\r') return fail(COCOA_E_ARG, "cocoa_model_save: method name holds a line break");
    std::string text = "COCOA-MODEL 1\nnumFeatures " + std::to_string(num_features) + "\nmethod " + name + "\nlambda " +
                       cocoa::jdouble::to_string(lambda) + "\nrounds " + std::to_string(rounds) + "\n";
    text.reserve(text.size() + (size_t)num_features * 24);
    for (int32_t j = 0; j < num_features; ++j) {
        text += cocoa::jdouble::to_string(w[j]);
        text += '\n';
    }
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(COCOA_E_IO, std::string("cocoa_model_save: cannot open ") + tmp + ": " + std::strerror(errno));
    const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
    if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return fail(COCOA_E_IO, std::string("cocoa_model_save: cannot write ") + path);
    }
    return COCOA_OK;
}

extern "C" int cocoa_model_load(const char* path, double** w_out, int32_t* num_features) {
    if (!path || !w_out || !num_features) return fail(COCOA_E_ARG, "cocoa_model_load: bad argument");
    *w_out = nullptr;
    *num_features = 0;
    FILE* f = std::fopen(path, "rb");
    if (!f) return fail(COCOA_E_IO, std::string("cocoa_model_load: cannot open ") + path + ": " + std::strerror(errno));
    std::string s;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, got);
    const bool rd_err = std::ferror(f) != 0;
    std::fclose(f);
    if (rd_err) return fail(COCOA_E_IO, std::string("cocoa_model_load: read error on ") + path);

    size_t pos = 0;
    std::string line, v;
    if (!next_line(s, pos, line) || line != "COCOA-MODEL 1")
        return fail(COCOA_E_PARSE, std::string("cocoa_model_load: ") + path + " is not a COCOA-MODEL 1 file");
    if (!next_line(s, pos, line) || !parse_field(line, "numFeatures", v) || v.empty() || v.size() > 10)
        return fail(COCOA_E_PARSE, "cocoa_model_load: bad numFeatures line");
    for (char c : v)
        if (c < '0' || c > '9') return fail(COCOA_E_PARSE, "cocoa_model_load: bad numFeatures line");
    const long long d = std::strtoll(v.c_str(), nullptr, 10);
    if (d < 1 || d > 2147483647LL) return fail(COCOA_E_PARSE, "cocoa_model_load: numFeatures out of range");
    if (!next_line(s, pos, line) || !parse_field(line, "method", v))
        return fail(COCOA_E_PARSE, "cocoa_model_load: bad method line");
    double lam = 0.0;
    if (!next_line(s, pos, line) || !parse_field(line, "lambda", v) || !parse_double(v, lam))
        return fail(COCOA_E_PARSE, "cocoa_model_load: bad lambda line");
    if (!next_line(s, pos, line) || !parse_field(line, "rounds", v))
        return fail(COCOA_E_PARSE, "cocoa_model_load: bad rounds line");
    double* w = (double*)std::malloc(sizeof(double) * (size_t)d);
    if (!w) return fail(COCOA_E_ARG, "cocoa_model_load: out of memory");
    for (long long j = 0; j < d; ++j) {
        if (!next_line(s, pos, line)) {
            std::free(w);
            return fail(COCOA_E_PARSE, "cocoa_model_load: " + std::to_string(j) + " weight lines, numFeatures is " +
                                           std::to_string(d));
        }
        if (!parse_double(line, w[j])) {
            std::free(w);
            return fail(COCOA_E_PARSE, "NumberFormatException: For input string: \"" + line + "\" (weight " +
                                           std::to_string(j) + ")");
        }
    }
    if (next_line(s, pos, line)) {
        std::free(w);
        return fail(COCOA_E_PARSE, "cocoa_model_load: more than numFeatures = " + std::to_string(d) + " weight lines");
    }
    *w_out = w;
    *num_features = (int32_t)d;
    return COCOA_OK;
}

extern "C" void cocoa_model_free(double* w) { std::free(w); }
