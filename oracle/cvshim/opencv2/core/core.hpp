/* Stand-in <opencv2/core/core.hpp> (test infrastructure): the old spelling of <opencv2/core.hpp>. */
#ifndef IVF_CVSHIM_CORE_CORE_HPP
#define IVF_CVSHIM_CORE_CORE_HPP
#include "../core.hpp"
#endif
