// KeyFrameDatabase_osg.cc — drop-in bodies for ORB_SLAM3::KeyFrameDatabase's members with call sites in this
// fork, on the MI355X path (ORB-SLAM3 tree built with -DORB_SLAM3_OSG).  Signatures:
// ref:include/KeyFrameDatabase.h.  The class gains one member under ORB_SLAM3_OSG,
//   std::shared_ptr<osg_orbslam3::KeyFrameDatabase<KeyFrame, Frame, Map>> mpOsg;
// and mvInvertedFile stays empty.  OsgHooks::device_vocabulary() is the vocabulary System uploaded with
// osg_vocabulary_load_text before it constructs the database.  DetectLoopCandidates, DetectCandidates and
// DetectBestCandidates have no caller in this fork and keep the reference's bodies (over an empty file).
#include "KeyFrameDatabase.h"
#include "osg_hooks_orbslam3.h"

namespace ORB_SLAM3 {

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary &voc)
    : mpVoc(&voc), mpOsg(std::make_shared<osg_orbslam3::KeyFrameDatabase<KeyFrame, Frame, Map>>(OsgHooks::device_vocabulary()))
{  // ref:src/KeyFrameDatabase.cc:32-35
}

void KeyFrameDatabase::add(KeyFrame *pKF) { mpOsg->add(pKF); }            // :42-50
void KeyFrameDatabase::erase(KeyFrame *pKF) { mpOsg->erase(pKF); }        // :57-78
void KeyFrameDatabase::clear() { mpOsg->clear(); }                        // :81-85
void KeyFrameDatabase::clearMap(Map *pMap) { mpOsg->clearMap(pMap); }     // :87-111

void KeyFrameDatabase::DetectNBestCandidates(KeyFrame *pKF, std::vector<KeyFrame *> &vpLoopCand,
                                             std::vector<KeyFrame *> &vpMergeCand, int nNumCandidates)
{  // :669-880
    mpOsg->DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates);
}

std::vector<KeyFrame *> KeyFrameDatabase::DetectRelocalizationCandidates(Frame *F, Map *pMap)
{  // :920-1031
    return mpOsg->DetectRelocalizationCandidates(F, pMap);
}

}  // namespace ORB_SLAM3
