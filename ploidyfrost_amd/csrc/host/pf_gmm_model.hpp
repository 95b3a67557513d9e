// pfh::GmmModel: the reference's GmmModel (src/GmmModel.hpp:5-49, src/GmmModel.cpp) with the EM iterations on the device
// (pf_gmm_upload / pf_gmm_fit, ../pf_gmm.hip).  Same method names and argument meaning; errors come back as a status plus
// error() instead of exit().  The readers run on the host -- they are the reference's text parsing, quirks included -- and
// need no device; emIterate() creates the device context on first use and fails without a gfx950 device (no CPU fit).
// borrow(): a model over values that are already resident in somebody else's context (pf_call_model_finish: the calling pipeline's
// own run) -- no second context, no upload, no host copy of the values.
#pragma once
#include <cstddef>
#include <ostream>
#include <string>
#include <vector>

#include "ploidyfrost_hip.h"

namespace pfh {

// one kernel density estimate (pf_gmm_density): the grid, the curve over it and the record of how it was made
struct Density {
    std::vector<double> x, density;
    pf_density_info info = {};
};

class GmmModel {
public:
    explicit GmmModel(int device = 0) : device_(device) {}
    ~GmmModel();
    GmmModel(const GmmModel &) = delete;
    GmmModel &operator=(const GmmModel &) = delete;

    void resize(size_t g);
    void setMThreshold(double m) { m_thre = m; }
    void setNThreshold(double n) { n_thre = n; }
    void setMaxIterNum(int i) { emMaxIter = i; }
    void setMaxDeltaNum(double i) { emMaxDelta = i; }
    int emIterate();   // 0 = ok
    double getLogLikelihood() const { return logLikelihood; }
    double computeAIC() {
        aic = (2 * ((double)gauss * 2 - 1) - 2 * logLikelihood) / (double)size();
        return aic;
    }
    double getAIC() const { return aic; }
    void readData(const std::vector<double> &v) { allele_fre = v; uploaded_ = false; }
    // the n values pf_gmm_fit finds resident in ctx (not owned, not destroyed); values() stays empty
    void borrow(pf_ctx *ctx, size_t n);
    size_t size() const { return borrowed_ ? borrowed_n_ : allele_fre.size(); }   // values the fit runs over
    // one record per emIterate() since the last clear_fits(): what output() prints, as numbers
    struct Fit {
        size_t gauss;
        std::vector<double> weights, means, vars;
        double loglik, aic;
        unsigned iterations;
    };
    const std::vector<Fit> &fits() const { return fits_; }
    void clear_fits() { fits_.clear(); }
    int readFreFile(const std::string &filename, const double &freq);
    int readCovFile(const std::string &prefix, const double &freq);
    // a plain column of numbers, what script/Drawfreq.R's read.table makes of its -f file: blank lines and lines that begin
    // with '#' are skipped, every other line is one finite number (strtod takes the whole token) or is refused with its number;
    // no frequency test and no doubled last value
    int readColumn(const std::string &filename);
    // the Gaussian kernel density of the values on the device (pf_gmm_density): 0 = ok
    int density(unsigned points, double adjust, Density &out);
    void output(std::ostream &os) const;
    void print() const;

    const std::vector<double> &values() const { return allele_fre; }
    const std::vector<double> &getWeights() const { return weights; }
    const std::vector<double> &getMeans() const { return means; }
    const std::vector<double> &getVars() const { return vars; }
    unsigned iterations() const { return iterations_; }
    const std::string &error() const { return err_; }
    pf_ctx *device_context() const { return ctx_; }

private:
    int fail(const std::string &m) { err_ = m; return 1; }
    int to_device();   // the context on first use, the values where the kernels read them
    std::vector<double> allele_fre;
    size_t gauss = 0;
    std::vector<double> weights, means, vars;
    double m_thre = 5.0, n_thre = 2.0;
    int emMaxIter = 1000;
    double emMaxDelta = 0.01;
    double logLikelihood = 0, aic = 0;
    unsigned iterations_ = 0;
    int device_;
    pf_ctx *ctx_ = nullptr;
    bool uploaded_ = false;
    bool borrowed_ = false;
    size_t borrowed_n_ = 0;
    std::vector<Fit> fits_;
    std::string err_;
};

// `PloidyFrost model` after option parsing (src/Main.cpp:644-692): fits gauss = lo .. hi, writes <outprefix>_model_result.txt
// *ploidy (optional): the value of the file's last line
int run_model(GmmModel &model, int lo, int hi, const std::string &outprefix, std::string &err, double *ploidy = nullptr);
// <outprefix>_allele_frequency_density.txt: "# values N bandwidth BW points P", then P rows x<TAB>density, every number %.17g
// (the doubles exactly; read.table and gnuplot skip the comment).  0 = ok
int write_density(const std::string &outprefix, const Density &d, std::string &err);
inline std::string density_file(const std::string &outprefix) { return outprefix + "_allele_frequency_density.txt"; }

}  // namespace pfh
