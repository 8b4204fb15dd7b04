/* Stand-in <opencv2/highgui/highgui.hpp> (test infrastructure): the reference's extractor includes it and uses nothing of it. */
#ifndef IVF_CVSHIM_HIGHGUI_HPP
#define IVF_CVSHIM_HIGHGUI_HPP
#include "../core.hpp"
#endif
