// options_plan_check NAME... -- VALUE...: every name x value through the option table of r2f_plan.cpp, answered as r2f_set_option
// answers (tests/test_options_host.py): "name <tab> value <tab> return code <tab> last error text" per call on stdout, and what an
// accepted value was stored as on stderr.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../include/r2f.h"
#include "../raw2film_amd/csrc/r2f_plan.h"

using namespace r2f;

int main(int argc, char** argv) {
    int sep = 1;
    while (sep < argc && strcmp(argv[sep], "--")) ++sep;
    plan::Options opt;
    std::string err;  // r2f_last_error: the text of the last failure
    for (int i = 1; i < sep; ++i)
        for (int j = sep + 1; j < argc; ++j) {
            const int value = (int)strtol(argv[j], nullptr, 10);
            int rc = R2F_OK;
            const plan::OptionRow* row = plan::find_option(argv[i]);
            if (!row)
                rc = R2F_EINVAL, err = std::string("unknown option ") + argv[i];
            else if (!plan::store_option(&opt, *row, value))
                rc = R2F_EINVAL, err = row->error;
            else
                fprintf(stderr, "stored\t%s\t%d\t%d\n", argv[i], value, opt.*row->field);
            printf("%s\t%d\t%d\t%s\n", argv[i], value, rc, err.c_str());
        }
    return 0;
}
